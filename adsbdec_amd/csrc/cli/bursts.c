/* bursts.c -- a capture's bursts: -U's gate behind -L's report, -K | -P keeping only them as a burst archive, -k decoding one. */
#include <hip/hip_runtime_api.h> /* -K | -P: the gathered pieces in a device buffer of this program's own */

#include "burst_archive.h"
#include "cli.h"

/* -L -U: the gate behind the report.  env: the device array of ceil(m / 28) floats the level call wrote.  keep (-K | -P; else NULL):
 * the table, its length and the threshold stay with the caller, who frees the table. */
struct kept_bursts {
    adsb_burst *tab;
    size_t n;
    float threshold;
};
static int print_bursts(adsb_decoder *dec, const adsb_level_report *rep, const float *d_env, uint64_t m, const struct burst_opts *u,
                        struct kept_bursts *keep)
{
    const size_t n_env = (size_t)((m + 27) / 28);
    const float median = adsb_level_percentile(rep, 0.5);
    if (median < 0) { /* (no sign-clear sample at all: nothing to take a median of) */
        printf("bursts 0 threshold none lead %u hang %u\n", u->lead, u->hang);
        if (keep) { /* -K: there is no threshold to gate with, so there is no archive to write; say so, and fail */
            fflush(stdout);
            fprintf(stderr, "-K: the capture has no sign-clear power sample, so the gate has no threshold: no archive is written\n");
            return 255;
        }
        return 0;
    }
    const float threshold = (float)(u->factor * median);
    size_t cap = 4096;
    adsb_burst *tab = (adsb_burst *)malloc(cap * sizeof *tab);
    long b = tab ? adsb_bursts_device(dec, d_env, n_env, threshold, u->lead, u->hang, tab, cap) : -1;
    if (tab && b > (long)cap) { /* grown once: B does not change between two calls on the same array */
        free(tab);
        cap = (size_t)b;
        tab = (adsb_burst *)malloc(cap * sizeof *tab);
        b = tab ? adsb_bursts_device(dec, d_env, n_env, threshold, u->lead, u->hang, tab, cap) : -1;
    }
    if (!tab) {
        fprintf(stderr, "out of memory for a table of %zu bursts\n", cap);
        return 255;
    }
    if (b < 0) {
        fprintf(stderr, "adsb_bursts_device() failed: %s\n", adsb_last_error(dec));
        return 255;
    }
    printf("bursts %ld threshold %.9g lead %u hang %u\n", b, (double)threshold, u->lead, u->hang);
    for (long i = 0; i < b; i++) {
        const uint64_t first = 28ull * tab[i].begin, end = 28ull * tab[i].end < m ? 28ull * tab[i].end : m;
        printf("%llu %llu %u %.9g\n", (unsigned long long)first, (unsigned long long)end, tab[i].hot, (double)tab[i].peak);
    }
    if (keep)
        keep->tab = tab, keep->n = (size_t)b, keep->threshold = threshold;
    else
        free(tab);
    return 0;
}

/* -K | -P: the pieces the table names, out of the capture the level call has read in HBM -- ONE gather call, ONE copy back, the
 * archive (burst_archive.h) of `kind`.  -K: adsb_gather_device out of the capture's own n_units units (`used` bytes).  -P, kind 12:
 * out of the capture's uint16 twin, packed to 12 bits while it is gathered, by the adsb_gather_pack12_* call of the file's flavour
 * (0: uint16; 1: -t fmt; 2: -p); a piece's own sample above 4095: no archive. */
static int keep_bursts(adsb_decoder *dec, const char *path, uint32_t kind, int flavour, int fmt, const void *d_in, size_t n_units, size_t used,
                       uint64_t m, const struct kept_bursts *k, const struct burst_opts *u)
{
    const int pack12 = kind == BRS_KIND_PACKED12_REAL;
    const char *layout = pack12 ? "adsb_gather_pack12_layout" : "adsb_gather_layout";
    const char *gather = !pack12 ? "adsb_gather_device" : flavour == 1 ? "adsb_gather_pack12_device_as" : flavour == 2 ? "adsb_gather_pack12_device_packed"
                                                                                                                       : "adsb_gather_pack12_device";
    brs_archive a;
    memset(&a, 0, sizeof a);
    a.kind = kind, a.sample_bytes = brs_sample_bytes(kind);
    a.n_units = n_units, a.m = m;
    a.threshold = k->threshold, a.lead = u->lead, a.hang = u->hang;
    a.n_bursts = k->n, a.bursts = k->tab;
    char why[512];
    uint64_t total = 0, over = 0;
    if ((pack12 ? adsb_gather_pack12_layout(m, k->tab, k->n, NULL, &total) : adsb_gather_layout(m, (int)a.sample_bytes, k->tab, k->n, NULL, &total)) != 0) {
        fprintf(stderr, "%s() failed: %s\n", layout, adsb_last_error(NULL));
        return 255;
    }
    void *d_out = NULL;
    unsigned char *out = (unsigned char *)malloc(total ? (size_t)total : 1);
    int rc = 255; /* (one way out: what was allocated here is released on it) */
    long got = -1;
    if (!out || (total && hipMalloc(&d_out, (size_t)total) != hipSuccess)) {
        d_out = NULL;
        fprintf(stderr, "cannot allocate the %llu bytes of the %zu bursts, on the host and on the device\n", (unsigned long long)total, k->n);
    } else if ((got = !pack12       ? adsb_gather_device(dec, d_in, used, (int)a.sample_bytes, m, k->tab, k->n, d_out, (size_t)total, NULL)
                      : flavour == 1 ? adsb_gather_pack12_device_as(dec, fmt, d_in, n_units, k->tab, k->n, d_out, (size_t)total, NULL, &over)
                      : flavour == 2 ? adsb_gather_pack12_device_packed(dec, d_in, n_units, k->tab, k->n, d_out, (size_t)total, NULL, &over)
                                     : adsb_gather_pack12_device(dec, d_in, n_units, k->tab, k->n, d_out, (size_t)total, NULL, &over)) < 0 ||
               (uint64_t)got != total) {
        fprintf(stderr, "%s() failed: %s\n", gather, got < 0 ? adsb_last_error(dec) : "another total than the layout's");
    } else if (over > 0) {
        fprintf(stderr, "-P: %llu samples inside the bursts are above 4095 and do not fit 12 bits: no archive is written (-K keeps all 16 bits)\n",
                (unsigned long long)over);
    } else if (total && hipMemcpy(out, d_out, (size_t)total, hipMemcpyDeviceToHost) != hipSuccess) {
        fprintf(stderr, "cannot copy the %llu bytes of the bursts back from the device\n", (unsigned long long)total);
    } else {
        a.payload = out, a.payload_bytes = total;
        if (brs_write(path, &a, why, sizeof why) != 0) {
            fprintf(stderr, "%s: %s\n", path, why);
        } else {
            fprintf(stderr, "kept %zu bursts, %llu of %llu bytes\n", k->n, (unsigned long long)total, (unsigned long long)(a.sample_bytes * m));
            rc = 0;
        }
    }
    if (d_out)
        (void)hipFree(d_out);
    free(out);
    return rc;
}

/* -L -U [-K | -P] behind run_level's report: the burst lines on stdout, then the archive.  flavour and fmt are run_level's kind of
 * input (0 uint16, 1 -t fmt, 2 -p, 3 -q fmt, 4 -w), d_in its n units (`used` bytes) on the device, m its power samples. */
int level_bursts(adsb_decoder *dec, const struct cli_options *o, const adsb_level_report *rep, const float *d_env, uint64_t m, int flavour,
                 int fmt, const void *d_in, size_t n, size_t used)
{
    const char *path = o->pack_out ? o->pack_out : o->archive_out;
    struct kept_bursts kept = {NULL, 0, 0};
    int rc = print_bursts(dec, rep, d_env, m, &o->burst, path ? &kept : NULL);
    if (rc == 0 && path) {
        /* (-P is refused with -q and -w: flavour 0, 1 or 2 there; -K with -t and -p: flavour 0, 3 or 4) */
        const uint32_t kind = o->pack_out ? BRS_KIND_PACKED12_REAL : flavour == 0 ? BRS_KIND_UINT16_REAL : flavour == 4 ? BRS_KIND_FLOAT32_POWER : (uint32_t)fmt;
        fflush(stdout);
        rc = keep_bursts(dec, path, kind, flavour, fmt, d_in, n, used, m, &kept, &o->burst);
    }
    free(kept.tab);
    return rc;
}

/* -k: decode a burst archive.  The pieces go through ONE adsb_decode_batch_host* call of the archive's kind on a flush handle (a piece
 * is far below the end-of-file horizon), pointers payload + offsets[i]; piece i's packets are its silent twin's, written in order with
 * g + 28 begin_i -- exact -- and ts + 28 begin_i: in the original stream ts lags g by what accepted frames have jumped
 * (demod.c:99,128,134), so this is the original's ts only up to those jumps.  The table is the sum of the pieces' tables. */
int run_archive(const struct cli_options *o)
{
    adsb_config cfg = cli_config(o);
    cfg.device = o->device;
    cli_one_device(&cfg.device);
    brs_archive a;
    char why[512];
    if (brs_read(o->filename, &a, why, sizeof why) != 0) {
        fprintf(stderr, "%s: %s\n", o->filename, why);
        return 255;
    }
    const size_t nb = (size_t)a.n_bursts;
    const void **piece = (const void **)calloc(nb + 1, sizeof *piece);
    size_t *n = (size_t *)calloc(nb + 1, sizeof *n);
    uint64_t *first = (uint64_t *)calloc(nb + 1, sizeof *first);
    adsb_stats *st = (adsb_stats *)calloc(nb + 1, sizeof *st);
    if (!piece || !n || !first || !st) {
        fprintf(stderr, "out of memory for the results of %zu pieces\n", nb);
        return 255;
    }
    for (size_t i = 0; i < nb; i++) {
        piece[i] = a.payload + a.offsets[i];
        n[i] = (size_t)brs_piece_units(&a, i); /* (kind 12: whole groups of 8 samples, a clipped last piece's fill included) */
    }
    const int peer = cli_wait_peer();
    if (peer == CLI_PEER_ENDED) {
        fflush(stderr);
        _exit(0);
    }
    if (peer == CLI_PEER_FAILED)
        return 255;
    adsb_decoder *dec = cli_create(&cfg);
    if (!dec)
        return 255;
    if (adsb_set_flush(dec, 1) != 0) {
        fprintf(stderr, "adsb_set_flush() failed: %s\n", adsb_last_error(dec));
        return 255;
    }
    const adsb_frame *fr = NULL;
    long total = 0;
    if (nb)
        total = a.kind == BRS_KIND_PACKED12_REAL   ? adsb_decode_batch_host_packed(dec, nb, piece, n, &fr, first, st)
                : a.kind == BRS_KIND_UINT16_REAL    ? adsb_decode_batch_host(dec, nb, (const uint16_t *const *)piece, n, &fr, first, st)
                : a.kind == BRS_KIND_FLOAT32_POWER ? adsb_decode_batch_host_power(dec, nb, (const float *const *)piece, n, &fr, first, st)
                                                   : adsb_decode_batch_host_iq(dec, (int)a.kind, nb, piece, n, &fr, first, st);
    if (total < 0) {
        fprintf(stderr, "the batch decode of the archive's %zu pieces failed: %s\n", nb, adsb_last_error(dec));
        return 255;
    }
    int rc = 0;
    adsb_stats sum;
    memset(&sum, 0, sizeof sum);
    adsb_frame *mine = (adsb_frame *)malloc((total ? (size_t)total : 1) * sizeof *mine);
    if (!mine) {
        fprintf(stderr, "out of memory for %ld packets\n", total);
        return 255;
    }
    for (size_t i = 0; i < nb; i++) {
        const uint64_t shift = 28ull * a.bursts[i].begin;
        for (uint64_t k = first[i]; k < first[i + 1]; k++) {
            mine[k] = fr[k];
            mine[k].g += shift, mine[k].ts += shift;
        }
        for (int j = 0; j < 3; j++)
            sum.try_[j] += st[i].try_[j], sum.ok[j] += st[i].ok[j];
        sum.fixed += st[i].fixed;
    }
    if (write_frames(&out_sink, mine, total, o->outformat) != 0)
        rc = 1;
    if (sink_close(&out_sink) != 0 && rc == 0)
        rc = 1;
    print_stats(&sum);
    cli_exit(rc);
}
