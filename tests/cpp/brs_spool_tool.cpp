// brs_spool_tool.cpp -- a stand-alone program around the burst archive writer that takes its payload from a spool file
// (csrc/cli/burst_archive.c brs_write_spooled: what the host program's record mode, -S -O, ends on), built with AddressSanitizer and
// UBSan by tests/test_burst_stream_cpu.py and run where no GPU is.  As tests/cpp/brs_tool.cpp it links neither the library nor the
// HIP runtime: adsb_gather_layout is csrc/gather.h's gather_layout behind host_abi.cpp's wrapper, restated here.
//
//     brs_spool_tool in.brs out.brs chunk    read in.brs; append its payload to out.brs.spool in writes of `chunk` bytes, as the
//                                            record mode appends piece after piece; write header, table and the spool to out.brs.tmp
//                                            and rename it: out.brs equals in.brs byte for byte, and no spool file is left
// A file the reader or the writer refuses: the reason on stderr, exit 1.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include <unistd.h>

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
    if (argc < 4 || atol(argv[3]) < 1) {
        fprintf(stderr, "usage: brs_spool_tool in.brs out.brs chunk\n");
        return 2;
    }
    brs_archive a;
    char why[512];
    if (brs_read(argv[1], &a, why, sizeof why) != 0) {
        fprintf(stderr, "%s: %s\n", argv[1], why);
        return 1;
    }
    const std::string out = argv[2], spool_path = out + ".spool", tmp_path = out + ".tmp";
    const uint64_t chunk = (uint64_t)atol(argv[3]);
    FILE *spool = fopen(spool_path.c_str(), "w+b");
    int rc = spool ? 0 : 1;
    for (uint64_t at = 0; rc == 0 && at < a.payload_bytes; at += chunk) {
        const size_t n = (size_t)(a.payload_bytes - at < chunk ? a.payload_bytes - at : chunk);
        rc = fwrite(a.payload + at, 1, n, spool) == n ? 0 : 1;
    }
    brs_archive b = a;
    b.payload = nullptr; // (the spooled writer does not read it)
    if (rc == 0 && brs_write_spooled(tmp_path.c_str(), &b, spool, why, sizeof why) != 0) {
        fprintf(stderr, "%s: %s\n", tmp_path.c_str(), why);
        rc = 1;
    }
    if (rc == 0 && brs_write_spooled(tmp_path.c_str(), &b, nullptr, why, sizeof why) == 0) {
        fprintf(stderr, "a NULL spool was not refused\n");
        rc = 1;
    }
    if (rc == 0 && rename(tmp_path.c_str(), out.c_str()) != 0)
        rc = 1;
    if (spool)
        fclose(spool);
    unlink(spool_path.c_str());
    brs_free(&a);
    return rc;
}
