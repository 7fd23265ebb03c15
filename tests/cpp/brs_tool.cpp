// brs_tool.cpp -- a stand-alone program around the host program's burst archive reader and writer (csrc/cli/burst_archive.c), built
// with AddressSanitizer and UBSan by tests/test_gather_cpu.py and run where no GPU is.  It links neither the library nor the HIP
// runtime: adsb_gather_layout is csrc/gather.h's gather_layout behind the wrapper host_abi.cpp puts around it, restated here
// (four lines), and adsb_last_error(NULL) shows what it refused.
//
//     brs_tool info in.brs            the header, the table with every piece's offset, and a checksum of the payload; exit 0
//     brs_tool copy in.brs out.brs    read, then write what was read: out.brs equals in.brs byte for byte
// A file the reader refuses: the reason on stderr, exit 1.
#include <cstdio>
#include <cstring>

#include "../../adsbdec_amd/csrc/gather.h"

extern "C" {
#include "../../adsbdec_amd/csrc/cli/burst_archive.h"
}

static char last_error[300];

extern "C" const char *adsb_last_error(const adsb_decoder *) { return last_error; }

extern "C" long adsb_gather_layout(uint64_t m, int sample_bytes, const adsb_burst *bursts, size_t n_bursts, uint64_t *offsets, uint64_t *total_bytes)
{
    char why[256];
    if (adsb::gather_layout(m, sample_bytes, bursts, n_bursts, nullptr, nullptr, nullptr, why, sizeof why) == 0)
        return adsb::gather_layout(m, sample_bytes, bursts, n_bursts, offsets, nullptr, total_bytes, why, sizeof why);
    snprintf(last_error, sizeof last_error, "adsb_gather_layout: %s", why);
    return -1;
}

int main(int argc, char **argv)
{
    if (argc < 3 || (strcmp(argv[1], "info") != 0 && strcmp(argv[1], "copy") != 0) || (strcmp(argv[1], "copy") == 0 && argc < 4)) {
        fprintf(stderr, "usage: brs_tool info in.brs | brs_tool copy in.brs out.brs\n");
        return 2;
    }
    brs_archive a;
    char why[512];
    if (brs_read(argv[2], &a, why, sizeof why) != 0) {
        fprintf(stderr, "%s: %s\n", argv[2], why);
        return 1;
    }
    int rc = 0;
    if (strcmp(argv[1], "copy") == 0) {
        if (brs_write(argv[3], &a, why, sizeof why) != 0) {
            fprintf(stderr, "%s: %s\n", argv[3], why);
            rc = 1;
        }
    } else {
        uint32_t tb;
        memcpy(&tb, &a.threshold, sizeof tb);
        printf("kind %u sample_bytes %u n_units %llu m %llu threshold_bits 0x%08x lead %u hang %u n_bursts %llu payload_bytes %llu\n", a.kind,
               a.sample_bytes, (unsigned long long)a.n_units, (unsigned long long)a.m, tb, a.lead, a.hang, (unsigned long long)a.n_bursts,
               (unsigned long long)a.payload_bytes);
        for (uint64_t i = 0; i < a.n_bursts; i++) {
            uint32_t pb;
            memcpy(&pb, &a.bursts[i].peak, sizeof pb);
            printf("burst %llu begin %u end %u hot %u peak_bits 0x%08x offset %llu\n", (unsigned long long)i, a.bursts[i].begin, a.bursts[i].end,
                   a.bursts[i].hot, pb, (unsigned long long)a.offsets[i]);
        }
        uint64_t h = 0xcbf29ce484222325ull; // FNV-1a over the payload
        for (uint64_t k = 0; k < a.payload_bytes; k++)
            h = (h ^ a.payload[k]) * 0x100000001b3ull;
        printf("total %llu payload_fnv1a 0x%016llx payload_aligned %d\n", (unsigned long long)a.offsets[a.n_bursts], (unsigned long long)h,
               (int)((uintptr_t)a.payload % 16 == 0));
    }
    brs_free(&a);
    return rc;
}
