/* record.c -- -S: gate a stream of any length and keep only its bursts.  A uint16 file or FIFO is read piece by piece; a piece is ONE
 * adsb_level_windows call (its report and its envelope), ONE adsb_bursts_slice_device call (the bursts the piece closes, joined across
 * the pieces by the carry) and, with -O, ONE adsb_gather_device call and one copy back of the closed bursts' samples, appended to a
 * spool file.  The device buffer holds the samples a later burst may still reach back to -- the open cluster, or the last `lead` runs
 * -- in front of the new piece: memory is bounded by the piece and by the longest burst, not by the stream.  At the end of the stream
 * (end of file, SIGINT / SIGTERM / SIGQUIT) one final call closes what is open and out.brs is written: header, table, the spool.
 *
 * Positions.  The stream's runs of 28 power samples (56 uint16 samples) count from 0.  The buffer `buf` starts at the stream's sample
 * 56 base_run - head, head = 16 where base_run > 0 (the six older pairs of run base_run's first power samples) and 0 at the stream's
 * start; every offset into it is a multiple of 8 samples, so every pointer handed to a call is 16-byte aligned.  The window call's
 * positions are REBASED by 56 (done - 1) samples: it gets first_sample = 40 and the edges 28 and 28 + m_new whatever `done` is, so its
 * first_sample + n < 2^32 never binds (a window's report and envelope depend on the samples, not on their positions: a multiple of 56
 * samples keeps first_sample % 8 and the edges on multiples of 28; tests/test_gpu_burst_stream.py holds two bases together). */
#include <hip/hip_runtime_api.h>

#include "burst_archive.h"
#include "cli.h"

#define RECORD_RETAIN_MOST ((uint64_t)64 << 20) /* samples: a retained part above this means the gate never closes */
#define RECORD_RUN_LIMIT ((uint64_t)1 << 31)    /* adsb_bursts_slice_*: a stream's runs stay below this */

struct dev_samples { /* a device array of uint16 samples, grown by release and allocate (nothing of it is kept) */
    uint16_t *p;
    size_t cap;
};
static int dev_reserve(struct dev_samples *b, size_t samples)
{
    if (samples <= b->cap)
        return 0;
    if (b->p)
        (void)hipFree(b->p);
    b->p = NULL, b->cap = 0;
    const size_t want = samples + samples / 4;
    if (hipMalloc((void **)&b->p, want * sizeof(uint16_t)) != hipSuccess) {
        fprintf(stderr, "cannot allocate %zu samples on the device\n", want);
        return -1;
    }
    b->cap = want;
    return 0;
}

struct record {
    adsb_decoder *dec;
    const struct record_opts *s;
    float threshold;
    int have_threshold, said_header;
    struct dev_samples buf, next; /* the samples in use; the array the retained part moves to */
    uint64_t base_run;            /* buf starts at sample 56 base_run - head of the stream */
    size_t held;                  /* samples in buf */
    adsb_burst_carry carry;
    adsb_burst *closed;           /* the bursts one piece closes */
    size_t closed_cap;
    adsb_burst *table;            /* every burst so far */
    size_t n_table, table_cap;
    float *d_env;                 /* piece floats */
    void *d_out;                  /* the gathered bytes of one piece */
    unsigned char *out;
    size_t out_cap;
    FILE *spool;
    uint64_t payload_bytes;
    uint64_t m_seen, n_seen;      /* power samples and uint16 samples of the stream so far */
};

static size_t head_of(uint64_t base_run) { return base_run ? 16 : 0; }

/* the bursts the piece closed: their lines, their place in the table, and with -O their samples into the spool */
static int record_closed(struct record *r, size_t n)
{
    if (!r->said_header) {
        printf("bursts threshold %.9g lead %u hang %u\n", (double)r->threshold, r->s->lead, r->s->hang);
        r->said_header = 1;
    }
    if (n == 0)
        return 0;
    for (size_t i = 0; i < n; i++) {
        const uint64_t first = 28ull * r->closed[i].begin, end = 28ull * r->closed[i].end < r->m_seen ? 28ull * r->closed[i].end : r->m_seen;
        printf("%llu %llu %u %.9g\n", (unsigned long long)first, (unsigned long long)end, r->closed[i].hot, (double)r->closed[i].peak);
    }
    if (r->n_table + n > r->table_cap) {
        const size_t want = 2 * (r->n_table + n);
        adsb_burst *t = (adsb_burst *)realloc(r->table, want * sizeof *t);
        if (!t) {
            fprintf(stderr, "out of memory for a table of %zu bursts\n", want);
            return 255;
        }
        r->table = t, r->table_cap = want;
    }
    memcpy(r->table + r->n_table, r->closed, n * sizeof *r->closed);
    r->n_table += n;
    if (!r->spool)
        return 0;
    /* the table rebased to the samples that buf holds from run base_run on; a burst begins at or behind base_run (the retained part) */
    const uint64_t m_held = (r->held - head_of(r->base_run)) / 4 * 2;
    for (size_t i = 0; i < n; i++) {
        if (r->closed[i].begin < r->base_run) {
            fprintf(stderr, "-S: a burst begins at run %u, in front of the retained run %llu\n", r->closed[i].begin, (unsigned long long)r->base_run);
            return 255;
        }
        r->closed[i].begin -= (uint32_t)r->base_run, r->closed[i].end -= (uint32_t)r->base_run;
    }
    uint64_t total = 0;
    if (adsb_gather_layout(m_held, 4, r->closed, n, NULL, &total) != 0) {
        fprintf(stderr, "adsb_gather_layout() failed: %s\n", adsb_last_error(NULL));
        return 255;
    }
    if (total > r->out_cap) {
        if (r->d_out)
            (void)hipFree(r->d_out);
        free(r->out);
        r->d_out = NULL, r->out_cap = 0;
        r->out = (unsigned char *)malloc((size_t)total);
        if (!r->out || hipMalloc(&r->d_out, (size_t)total) != hipSuccess) {
            fprintf(stderr, "cannot allocate the %llu bytes of %zu bursts, on the host and on the device\n", (unsigned long long)total, n);
            return 255;
        }
        r->out_cap = (size_t)total;
    }
    const long got = adsb_gather_device(r->dec, r->buf.p + head_of(r->base_run), (size_t)(2 * m_held) * sizeof(uint16_t), 4, m_held, r->closed, n,
                                        r->d_out, (size_t)total, NULL);
    if (got < 0 || (uint64_t)got != total) {
        fprintf(stderr, "adsb_gather_device() failed: %s\n", got < 0 ? adsb_last_error(r->dec) : "another total than the layout's");
        return 255;
    }
    if (hipMemcpy(r->out, r->d_out, (size_t)total, hipMemcpyDeviceToHost) != hipSuccess) {
        fprintf(stderr, "cannot copy the %llu bytes of the bursts back from the device\n", (unsigned long long)total);
        return 255;
    }
    if (fwrite(r->out, 1, (size_t)total, r->spool) != (size_t)total) {
        fprintf(stderr, "cannot write the spool file: %s\n", strerror(errno));
        return 255;
    }
    r->payload_bytes += total;
    return 0;
}

/* One piece: n_new samples in host memory at x (0 at the end of a stream whose length is whole pieces), the last one where `final`. */
static int record_piece(struct record *r, const uint16_t *x, size_t n_new, int final)
{
    const uint64_t done = r->carry.runs, m_new = 2 * (uint64_t)(n_new / 4);
    const size_t n_env = (size_t)((m_new + 27) / 28);
    if (n_new) {
        if (hipMemcpy(r->buf.p + r->held, x, n_new * sizeof(uint16_t), hipMemcpyHostToDevice) != hipSuccess) {
            fprintf(stderr, "cannot bring a piece of %zu samples to the device\n", n_new);
            return 255;
        }
    }
    if (m_new) {
        const size_t front = done ? 16 : 0; /* the 16 samples before the piece: the retained part holds them */
        const uint64_t first_sample = done ? 40 : 0, edges[2] = {done ? 28 : 0, (done ? 28 : 0) + m_new};
        adsb_level_report *rep = (adsb_level_report *)malloc(sizeof *rep);
        if (!rep) {
            fprintf(stderr, "out of memory for a level report\n");
            return 255;
        }
        if (adsb_level_windows(r->dec, r->buf.p + r->held - front, first_sample, n_new + front, 1, edges, rep, r->d_env, n_env) < 0) {
            fprintf(stderr, "adsb_level_windows() failed: %s\n", adsb_last_error(r->dec));
            return 255;
        }
        if (!r->have_threshold) { /* the first piece decides, so that the header's threshold is true of every burst */
            const float median = adsb_level_percentile(rep, 0.5);
            if (median < 0) {
                fprintf(stderr, "-S: the first piece has no sign-clear power sample, so the gate has no threshold: no archive is written\n");
                return 255;
            }
            r->threshold = r->s->absolute ? (float)r->s->factor : (float)(r->s->factor * median);
            r->have_threshold = 1;
        }
        free(rep);
    }
    r->held += n_new, r->m_seen += m_new, r->n_seen += n_new;
    if (!r->have_threshold) /* (a stream without one power sample) */
        r->threshold = r->s->absolute ? (float)r->s->factor : 0.0f, r->have_threshold = r->s->absolute;
    if (!r->have_threshold) {
        fprintf(stderr, "-S: the stream has no power sample, so the gate has no threshold: no archive is written\n");
        return 255;
    }
    adsb_burst_carry out;
    long b = adsb_bursts_slice_device(r->dec, r->d_env, n_env, r->threshold, r->s->lead, r->s->hang, &r->carry, final, r->closed, r->closed_cap, &out);
    if (b > (long)r->closed_cap) { /* grown, and the same call again with the same carry in */
        free(r->closed);
        r->closed_cap = (size_t)b;
        r->closed = (adsb_burst *)malloc(r->closed_cap * sizeof *r->closed);
        if (!r->closed) {
            fprintf(stderr, "out of memory for a table of %ld bursts\n", b);
            return 255;
        }
        b = adsb_bursts_slice_device(r->dec, r->d_env, n_env, r->threshold, r->s->lead, r->s->hang, &r->carry, final, r->closed, r->closed_cap, &out);
    }
    if (b < 0) {
        fprintf(stderr, "adsb_bursts_slice_device() failed: %s\n", adsb_last_error(r->dec));
        return 255;
    }
    r->carry = out;
    return record_closed(r, (size_t)b);
}

/* Behind a piece that is not the last: keep the samples from 16 before run min(carry.first - lead, runs - lead) on -- the open cluster,
 * or the last `lead` runs, which a later burst's begin reaches back to -- at the front of the other array, and make room for a piece. */
static int record_retain(struct record *r, size_t piece_samples)
{
    const uint64_t runs = r->carry.runs, lead = r->s->lead;
    uint64_t from = r->carry.open && r->carry.first < runs ? r->carry.first : runs;
    from = from > lead ? from - lead : 0;
    if (from < r->base_run)
        from = r->base_run;
    const size_t src = head_of(r->base_run) + (size_t)(56 * (from - r->base_run)) - head_of(from), kept = r->held - src;
    const char *few = getenv("ADSB_CLI_RECORD_RETAIN"); /* (for tests: the most samples retained, so that a small file reaches it) */
    const uint64_t most = few && atoll(few) > 0 && (uint64_t)atoll(few) < RECORD_RETAIN_MOST ? (uint64_t)atoll(few) : RECORD_RETAIN_MOST;
    if (kept > most) {
        fprintf(stderr, "-S: a burst is open over more than %llu samples: the gate never closes at this threshold; raise the factor\n",
                (unsigned long long)most);
        return 255;
    }
    if (src == 0 && r->buf.cap >= kept + piece_samples) /* (the whole array is kept, and it takes one more piece) */
        return 0;
    if (dev_reserve(&r->next, kept + piece_samples) != 0)
        return 255;
    if (kept && hipMemcpy(r->next.p, r->buf.p + src, kept * sizeof(uint16_t), hipMemcpyDeviceToDevice) != hipSuccess) {
        fprintf(stderr, "cannot move the %zu retained samples on the device\n", kept);
        return 255;
    }
    const struct dev_samples t = r->buf;
    r->buf = r->next, r->next = t;
    r->base_run = from, r->held = kept;
    return 0;
}

int run_record(const struct cli_options *o)
{
    const struct record_opts *s = &o->record;
    int device = o->device;
    const int fd = open(o->filename, O_RDONLY);
    if (fd < 0) {
        fprintf(stderr, "%s: cannot read: %s\n", o->filename, strerror(errno));
        return 255;
    }
    install_signals();
    struct record r;
    memset(&r, 0, sizeof r);
    r.s = s;
    r.dec = cli_create_on(&device);
    if (!r.dec)
        return 255;
    const uint64_t piece = s->piece; /* runs */
    const size_t piece_samples = (size_t)(56 * piece);
    uint16_t *x = (uint16_t *)malloc(piece_samples * sizeof(uint16_t) + 1);
    r.closed_cap = 4096;
    r.closed = (adsb_burst *)malloc(r.closed_cap * sizeof *r.closed);
    if (!x || !r.closed) {
        fprintf(stderr, "out of memory for pieces of %zu samples\n", piece_samples);
        return 255;
    }
    if (hipSetDevice(device < 0 ? 0 : device) != hipSuccess || dev_reserve(&r.buf, piece_samples + 16) != 0 ||
        hipMalloc((void **)&r.d_env, (size_t)piece * sizeof(float)) != hipSuccess) {
        fprintf(stderr, "cannot allocate a piece of %zu samples and its envelope on the device\n", piece_samples);
        return 255;
    }
    char spool_path[4096] = "", tmp_path[4096] = "";
    if (o->record_out) {
        if (snprintf(spool_path, sizeof spool_path, "%s.spool", o->record_out) >= (int)sizeof spool_path ||
            snprintf(tmp_path, sizeof tmp_path, "%s.tmp", o->record_out) >= (int)sizeof tmp_path) {
            fprintf(stderr, "-O: the path is too long\n");
            return 255;
        }
        r.spool = fopen(spool_path, "w+b");
        if (!r.spool) {
            fprintf(stderr, "%s: cannot create the spool file: %s\n", spool_path, strerror(errno));
            return 255;
        }
    }
    int rc = 0, too_long = 0;
    const int timing = cli_timing(); /* ADSB_CLI_TIMING: where the wall time went, a line on stderr at the end */
    const double t_start = now_ms();
    double t_read = 0, t_device = 0;
    for (int final = 0; rc == 0 && !final;) {
        /* a stream that reaches 2^31 runs ends there, as if the file ended */
        const uint64_t room = RECORD_RUN_LIMIT - 1 - r.carry.runs;
        const size_t want = (size_t)(56 * (room < piece ? room : piece)) * sizeof(uint16_t);
        const double t0 = now_ms();
        const size_t bytes = stop_requested ? 0 : read_full(fd, x, want);
        const double t1 = now_ms();
        too_long = room < piece && bytes == want;
        final = bytes < want || too_long || stop_requested;
        const size_t n_new = bytes / sizeof(uint16_t);
        if (final && bytes - (n_new / 4 * 4) * sizeof(uint16_t))
            fprintf(stderr, "%zu trailing bytes ignored (the reference reads four samples at a time)\n", bytes - (n_new / 4 * 4) * sizeof(uint16_t));
        rc = record_piece(&r, x, n_new, final);
        if (rc == 0 && !final)
            rc = record_retain(&r, piece_samples);
        t_read += t1 - t0, t_device += now_ms() - t1;
    }
    fflush(stdout);
    if (timing)
        fprintf(stderr, "[record] reading %.1f ms, pieces on the device (level, gate, gather, spool, lines) %.1f ms, %.1f ms since the GPU was open\n",
                t_read, t_device, now_ms() - t_start);
    if (rc == 0 && r.spool) {
        brs_archive a;
        memset(&a, 0, sizeof a);
        a.kind = BRS_KIND_UINT16_REAL, a.sample_bytes = brs_sample_bytes(a.kind);
        a.n_units = r.n_seen, a.m = r.m_seen;
        a.threshold = r.threshold, a.lead = s->lead, a.hang = s->hang;
        a.n_bursts = r.n_table, a.bursts = r.table, a.payload_bytes = r.payload_bytes;
        char why[512];
        if (brs_write_spooled(tmp_path, &a, r.spool, why, sizeof why) != 0) {
            fprintf(stderr, "%s: %s\n", o->record_out, why);
            rc = 255;
        } else if (rename(tmp_path, o->record_out) != 0) {
            fprintf(stderr, "%s: cannot rename the finished archive to it: %s\n", o->record_out, strerror(errno));
            rc = 255;
        } else {
            fprintf(stderr, "kept %zu bursts, %llu of %llu bytes\n", r.n_table, (unsigned long long)r.payload_bytes, (unsigned long long)(4 * r.m_seen));
        }
    }
    if (r.spool) {
        fclose(r.spool);
        (void)unlink(spool_path);
        if (rc)
            (void)unlink(tmp_path);
    }
    if (rc)
        return rc;
    if (too_long) {
        fprintf(stderr, "-S: the stream reached 2^31 runs (%llu power samples): it ends there, and what follows is not recorded\n",
                (unsigned long long)r.m_seen);
        fflush(stderr);
        cli_exit(255);
    }
    cli_exit(0);
}
