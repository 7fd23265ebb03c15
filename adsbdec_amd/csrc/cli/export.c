/* export.c -- -W: the file's power samples into the file named; nothing is decoded.  A piece of a uint16 file is EXPORT_PIECE power
 * samples (a multiple of 28: about 4 Mi samples) behind the last 16 samples of the piece before it; an IQ piece is EXPORT_PIECE
 * complex samples. */
#include <hip/hip_runtime_api.h> /* -W -q: a device buffer of this program's own (three calls) */

#include "cli.h"

#define EXPORT_PIECE ((uint64_t)28 * 74898)
#define EXPORT_OVERLAP 16

int run_export(const struct cli_options *o)
{
    const char *outpath = o->export_path;
    const int qtype = (int)o->qtype;
    int device = o->device;
    install_signals();
    const int fd = open(o->filename, O_RDONLY);
    if (fd < 0) {
        fprintf(stderr, "%s: cannot read: %s\n", o->filename, strerror(errno));
        return 255;
    }
    adsb_decoder *dec = cli_create_on(&device);
    if (!dec)
        return 255;
    FILE *out = fopen(outpath, "wb"); /* (behind adsb_create: no empty file is left where no GPU is) */
    if (!out) {
        fprintf(stderr, "%s: cannot write: %s\n", outpath, strerror(errno));
        return 255;
    }
    int rc = 0;
    float *pw = (float *)malloc(EXPORT_PIECE * sizeof(float));
    if (!o->iq) {
        uint16_t *buf = (uint16_t *)malloc((EXPORT_OVERLAP + 2 * EXPORT_PIECE) * sizeof(uint16_t));
        if (!buf || !pw) {
            fprintf(stderr, "out of memory for the export buffers\n");
            return 255;
        }
        for (uint64_t k = 0; rc == 0 && !stop_requested; k++) {
            const size_t bytes = read_full(fd, buf + EXPORT_OVERLAP, 2 * EXPORT_PIECE * sizeof(uint16_t));
            const size_t have = bytes / 2; /* (a trailing odd byte is dropped, as decodeiq(iqbuff, n / 2) drops it, air.c:239) */
            const size_t lead = k ? EXPORT_OVERLAP : 0;
            const uint64_t m_begin = k * EXPORT_PIECE, m_end = m_begin + 2 * (have / 4);
            const long got = adsb_power_window_host(dec, buf + EXPORT_OVERLAP - lead, 2 * m_begin - lead, have + lead, m_begin, m_end, pw, EXPORT_PIECE);
            if (got < 0) {
                fprintf(stderr, "adsb_power_window_host() failed: %s\n", adsb_last_error(dec));
                rc = 255;
            } else if (fwrite(pw, sizeof(float), (size_t)got, out) != (size_t)got) {
                fprintf(stderr, "%s: cannot write\n", outpath);
                rc = 1;
            }
            if (have < 2 * EXPORT_PIECE) {
                if (rc == 0 && (have % 4 || bytes % 2))
                    fprintf(stderr, "%zu trailing bytes ignored (the reference reads four samples at a time)\n", (have % 4) * 2 + bytes % 2);
                break;
            }
            memcpy(buf, buf + 2 * EXPORT_PIECE, EXPORT_OVERLAP * sizeof(uint16_t)); /* the next piece's overlap */
        }
    } else {
        const size_t elem = adsb_iq_bytes(qtype, 1);
        void *buf = malloc(EXPORT_PIECE * elem), *d_in = NULL, *d_out = NULL;
        if (!buf || !pw) {
            fprintf(stderr, "out of memory for the export buffers\n");
            return 255;
        }
        if (hipSetDevice(device < 0 ? 0 : device) != hipSuccess || hipMalloc(&d_in, EXPORT_PIECE * elem) != hipSuccess ||
            hipMalloc(&d_out, EXPORT_PIECE * sizeof(float)) != hipSuccess) {
            fprintf(stderr, "cannot allocate the device buffers of the export\n");
            return 255;
        }
        while (rc == 0 && !stop_requested) { /* (every piece a call of its own, no stream position: any length) */
            const size_t bytes = read_full(fd, buf, EXPORT_PIECE * elem);
            const size_t have = bytes / elem;
            long got = 0;
            if (have && hipMemcpy(d_in, buf, have * elem, hipMemcpyHostToDevice) != hipSuccess) {
                fprintf(stderr, "copying a piece to the device failed\n");
                rc = 255;
            } else if (have && (got = adsb_power_device_iq(dec, qtype, d_in, have, (float *)d_out, EXPORT_PIECE)) < 0) {
                fprintf(stderr, "adsb_power_device_iq() failed: %s\n", adsb_last_error(dec));
                rc = 255;
            } else if (got && hipMemcpy(pw, d_out, (size_t)got * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) {
                fprintf(stderr, "copying a piece from the device failed\n");
                rc = 255;
            } else if (fwrite(pw, sizeof(float), (size_t)got, out) != (size_t)got) {
                fprintf(stderr, "%s: cannot write\n", outpath);
                rc = 1;
            }
            if (bytes < EXPORT_PIECE * elem) {
                if (rc == 0 && bytes % elem)
                    fprintf(stderr, "%zu trailing bytes ignored (not a whole %zu-byte sample)\n", bytes % elem, elem);
                break;
            }
        }
        adsb_format_report rep;
        if (rc == 0 && qtype == ADSB_FMT_FLOAT32_IQ && adsb_get_format_report(dec, &rep) == 0 && rep.inexact + rep.clamped > 0)
            fprintf(stderr, "%llu of %llu float scalars were rounded to the int16 grid (%llu clamped): expected of a float32 IQ capture\n",
                    (unsigned long long)(rep.inexact + rep.clamped), (unsigned long long)rep.converted, (unsigned long long)rep.clamped);
    }
    if (fclose(out) != 0 && rc == 0) {
        fprintf(stderr, "%s: cannot write\n", outpath);
        rc = 1;
    }
    if (stop_requested && rc == 0) { /* (a signal ended the loop between two pieces) */
        fprintf(stderr, "%s: interrupted: the file holds the pieces written so far, not the whole export\n", outpath);
        rc = 1;
    }
    cli_exit(rc);
}
