/* stream.c -- the plain decode: one capture of -f, streamed through one GPU.
 *
 * fileInput (air.c:217-246) reads 2 MiB at a time into one buffer and decodes it before the
 * next read().  Here a reader thread fills a ring of 32 MiB buffers from the moment the
 * program starts -- so the file is being read while the GPU runtime initialises (~0.2 s) --
 * and the main thread hands each filled buffer to adsb_push_async(), which overlaps the
 * host-to-device copy of one buffer with the scan of the previous one. */
#include <pthread.h>
#include <sys/mman.h>
#include <time.h>

#include "cli.h"

#define BUF_SAMPLES (16u * 1024u * 1024u)
#define RING_MAX_BYTES (1024ull * 1024ull * 1024ull)

typedef struct {
    uint16_t *buf;
    size_t bytes; /* valid bytes once filled */
    int filled;
    int registered;
    int ready;    /* filled, and page-locked if that was asked for: the main thread may push it */
} ring_slot;

typedef struct {
    int fd, nbuf, failed, use_register;
    /* bytes per ring buffer: BUF_SAMPLES samples, as uint16 (32 MiB), packed 12-bit with -p (24 MiB: whole 12-byte groups), or what
     * adsb_format_bytes / adsb_iq_bytes say for -t 1 | 3 / -q; -w: float32 */
    size_t buf_bytes;
    double t_reg;
    ring_slot *slot;
    pthread_mutex_t mu;
    pthread_cond_t cv;
} ring;

static void *reader_main(void *arg)
{
    ring *r = (ring *)arg;
    const size_t cap = r->buf_bytes;
    for (int k = 0;; k++) {
        ring_slot *s = &r->slot[k % r->nbuf];
        pthread_mutex_lock(&r->mu);
        while (s->filled)
            pthread_cond_wait(&r->cv, &r->mu);
        pthread_mutex_unlock(&r->mu);
        if (!s->buf) {
            /* 2 MiB-aligned and marked for transparent huge pages: first-touching 32 MiB then takes 16
             * page faults instead of 8192 -- the faults of a 4 KiB-page buffer hold the address-space
             * lock that the GPU runtime's start-up (hundreds of mmaps) needs at the same moment, and
             * were measured to slow it down by more than the overlap gained */
            if (posix_memalign((void **)&s->buf, 2u << 20, cap) != 0) {
                s->buf = NULL;
                r->failed = 1;
            } else {
                madvise(s->buf, cap, MADV_HUGEPAGE);
            }
        }
        const size_t got = s->buf ? read_full(r->fd, s->buf, cap) : 0; /* fill the buffer: only the last one of a file is short */
        pthread_mutex_lock(&r->mu);
        s->bytes = got;
        s->filled = 1;
        pthread_cond_broadcast(&r->cv);
        pthread_mutex_unlock(&r->mu);
        if (got < cap)
            return NULL; /* end of file (or an error: the run ends there, air.c:236-237) */
    }
}

/* Started once the GPU runtime is up: page-locks the filled buffers in ring order (each one
 * once), so that buffer k+1 is being locked while buffer k is pushed. */
static void *locker_main(void *arg)
{
    ring *r = (ring *)arg;
    for (int k = 0;; k++) {
        ring_slot *s = &r->slot[k % r->nbuf];
        pthread_mutex_lock(&r->mu);
        while (!s->filled || s->ready)
            pthread_cond_wait(&r->cv, &r->mu);
        pthread_mutex_unlock(&r->mu);
        const size_t bytes = s->bytes;
        if (r->use_register && !s->registered && s->buf && bytes >= 2) {
            const double t0 = now_ms();
            s->registered = adsb_host_register(s->buf, r->buf_bytes) == 0;
            r->t_reg += now_ms() - t0;
        }
        pthread_mutex_lock(&r->mu);
        s->ready = 1;
        pthread_cond_broadcast(&r->cv);
        pthread_mutex_unlock(&r->mu);
        if (bytes < r->buf_bytes)
            return NULL;
    }
}

/* pthread_cond_wait that wakes up ten times a second to look at stop_requested (a signal does not wake a condition wait) */
static void cond_wait_tick(pthread_cond_t *cv, pthread_mutex_t *mu)
{
    struct timespec ts;
    clock_gettime(CLOCK_REALTIME, &ts);
    ts.tv_nsec += 100 * 1000 * 1000;
    if (ts.tv_nsec >= 1000000000L) {
        ts.tv_sec++;
        ts.tv_nsec -= 1000000000L;
    }
    pthread_cond_timedwait(cv, mu, &ts);
}

static int flush_frames(adsb_decoder *dec, int outformat)
{
    const adsb_frame *fr; /* the handle's own queue: formatted where it lies */
    const long n = adsb_take(dec, &fr);
    if (n < 0)
        return -1;
    return write_frames(&out_sink, fr, n, outformat);
}

/* one buffer of the ring into the handle, by the call of the input's kind; async where the buffer is page-locked */
static int push_slot(adsb_decoder *dec, const struct cli_options *o, const ring_slot *s, size_t n_samples)
{
    if (o->power)
        return s->registered ? adsb_push_power_async(dec, (const float *)s->buf, n_samples) : adsb_push_power(dec, (const float *)s->buf, n_samples);
    if (o->iq)
        return s->registered ? adsb_push_iq_async(dec, (int)o->qtype, s->buf, n_samples) : adsb_push_iq(dec, (int)o->qtype, s->buf, n_samples);
    if (o->packed)
        return s->registered ? adsb_push_packed_async(dec, s->buf, n_samples) : adsb_push_packed(dec, s->buf, n_samples);
    if (o->converted)
        return s->registered ? adsb_push_async_as(dec, (int)o->stype, s->buf, n_samples) : adsb_push_as(dec, (int)o->stype, s->buf, n_samples);
    return s->registered ? adsb_push_async(dec, s->buf, n_samples) : adsb_push(dec, s->buf, n_samples);
}

int run_stream(const struct cli_options *o)
{
    const int packed = o->packed, power = o->power, iq = o->iq, converted = o->converted, outformat = o->outformat;
    const size_t elem = power ? sizeof(float) : iq ? adsb_iq_bytes((int)o->qtype, 1) : converted ? adsb_format_bytes((int)o->stype, 1) : 2; /* (host arithmetic: no GPU call) */
    const int timing = cli_timing();
    int device = o->device;
    cli_one_device(&device); /* before the runtime's first call */
    const int use_register = !(getenv("ADSB_CLI_REGISTER") && atoi(getenv("ADSB_CLI_REGISTER")) == 0);
    const double t_start = now_ms();

    /* start reading before anything touches the GPU.  (static: a run that fails below returns, and the process ends through
     * exit(), while the reader may still be filling the ring) */
    static ring rg;
    rg.buf_bytes = power       ? sizeof(float) * (BUF_SAMPLES / 2)
                   : iq        ? adsb_iq_bytes((int)o->qtype, BUF_SAMPLES / 2)
                   : converted ? adsb_format_bytes((int)o->stype, BUF_SAMPLES)
                   : packed    ? (size_t)BUF_SAMPLES / 8 * 12
                               : (size_t)BUF_SAMPLES * 2;
    pthread_t reader;
    int have_reader = 0;
    rg.fd = open(o->filename, O_RDONLY);
    if (rg.fd >= 0) { /* an unopenable file ends the run silently (air.c:225-228) */
        struct stat sb;
        unsigned long long size = (fstat(rg.fd, &sb) == 0 && sb.st_size > 0) ? (unsigned long long)sb.st_size : 0;
        unsigned long long ring_max = RING_MAX_BYTES;
        if (getenv("ADSB_CLI_RING_MB") && atoll(getenv("ADSB_CLI_RING_MB")) >= 96) /* (measurement knob of this program, not of the library) */
            ring_max = (unsigned long long)atoll(getenv("ADSB_CLI_RING_MB")) << 20;
        if (size > ring_max || size == 0)
            size = ring_max; /* pipes and large files: a bounded ring, the reader waits for free buffers */
        rg.nbuf = (int)(size / rg.buf_bytes) + 2;
        if (rg.nbuf < 3)
            rg.nbuf = 3;
        rg.slot = (ring_slot *)calloc((size_t)rg.nbuf, sizeof *rg.slot);
        pthread_mutex_init(&rg.mu, NULL);
        pthread_cond_init(&rg.cv, NULL);
        have_reader = rg.slot && pthread_create(&reader, NULL, reader_main, &rg) == 0;
    }

    /* the peer, while the file is being read */
    const int peer = cli_wait_peer();
    if (peer == CLI_PEER_ENDED) {
        fflush(stderr);
        _exit(0);
    }
    if (peer == CLI_PEER_FAILED)
        return 255;

    adsb_config cfg = cli_config(o);
    cfg.device = device; /* (-1: the current one; after the narrowing above, 0) */
    cfg.warm_start = 1;  /* a one-shot process: the runtime's first-use costs are paid inside adsb_create, beside its other work */
    adsb_decoder *dec = cli_create(&cfg);
    if (!dec)
        return 255;
    if (o->flush && adsb_set_flush(dec, 1) != 0) { /* -E: the stream ends as its silent twin does (and below 2^32 samples: a long stream has no flush) */
        fprintf(stderr, "adsb_set_flush() failed: %s\n", adsb_last_error(dec));
        return 255;
    }
    if (!o->flush && !iq && !power && adsb_set_long_stream(dec, 1) != 0) { /* always: the reference reads a file of any length (its counter wraps, air.c:34) */
        fprintf(stderr, "adsb_set_long_stream() failed: %s\n", adsb_last_error(dec));
        return 255;
    }
    const double t_init = now_ms();

    int rc = 0;
    pthread_t locker;
    rg.use_register = use_register;
    if (have_reader && pthread_create(&locker, NULL, locker_main, &rg) != 0)
        have_reader = 0;
    int stopped = 0, n_push = 0;
    double t_wait_ring = 0, t_push = 0, t_flush = 0, t_finish = 0;
    if (have_reader) {
        int prev = -1;
        for (int k = 0;; k++) {
            ring_slot *s = &rg.slot[k % rg.nbuf];
            const double t_w0 = now_ms();
            pthread_mutex_lock(&rg.mu);
            while (!s->ready && !stop_requested)
                cond_wait_tick(&rg.cv, &rg.mu);
            const int reader_failed = rg.failed; /* (written under the mutex by the reader) */
            const int is_ready = s->ready;
            pthread_mutex_unlock(&rg.mu);
            t_wait_ring += now_ms() - t_w0;
            if (stop_requested && !is_ready) {
                stopped = 1; /* SIGINT / SIGTERM / SIGQUIT: no more pushes; what is in the decoder is finished below */
                break;
            }
            if (reader_failed) {
                fprintf(stderr, "out of memory for the read buffers\n");
                rc = 255;
                break;
            }
            const size_t bytes = s->bytes;
            /* a trailing odd byte is dropped, like decodeiq(iqbuff, n / 2) (air.c:239); packed: a trailing partial group (only the
             * last buffer can have one: a full buffer is whole groups) */
            const size_t n_samples = packed ? bytes / 12 * 8 : bytes / elem;
            if ((converted || iq || power) && bytes % elem)
                fprintf(stderr, "%zu trailing bytes ignored (not a whole %zu-byte sample)\n", bytes % elem, elem);
            if (packed && bytes % 12)
                fprintf(stderr, "%zu trailing bytes ignored (not a whole 12-byte group of packed samples)\n", bytes % 12);
            if (n_samples) {
                const double t_p0 = now_ms();
                const int prc = push_slot(dec, o, s, n_samples);
                t_push += now_ms() - t_p0;
                n_push++;
                if (timing > 1)
                    fprintf(stderr, "  push %d (%s): %.2f ms at +%.1f ms\n", n_push, s->registered ? "async" : "sync", now_ms() - t_p0, t_p0 - t_init);
                if (prc != 0) {
                    fprintf(stderr, "adsb_push() failed: %s\n", adsb_last_error(dec));
                    rc = 255;
                    break;
                }
                const double t_f0 = now_ms();
                const int frc = flush_frames(dec, outformat);
                t_flush += now_ms() - t_f0;
                if (frc != 0) { /* stdout is gone (EPIPE, disk full): stop, and say so */
                    rc = 1;
                    break;
                }
            }
            if (prev >= 0) { /* the buffer of the previous push is free again (adsb_push_async's contract) */
                pthread_mutex_lock(&rg.mu);
                rg.slot[prev].ready = 0;
                rg.slot[prev].filled = 0;
                pthread_cond_broadcast(&rg.cv);
                pthread_mutex_unlock(&rg.mu);
            }
            prev = k % rg.nbuf;
            if (bytes < rg.buf_bytes)
                break; /* that was the last buffer */
            if (stop_requested) {
                stopped = 1;
                break;
            }
        }
        const double t_fin0 = now_ms();
        if (rc == 0 && adsb_finish(dec) != 0) {
            fprintf(stderr, "adsb_finish() failed: %s\n", adsb_last_error(dec));
            rc = 255;
        }
        if (flush_frames(dec, outformat) != 0 && rc == 0)
            rc = 1;
        t_finish = now_ms() - t_fin0;
        if (sink_close(&out_sink) != 0 && rc == 0)
            rc = 1; /* the last block did not reach the file (ENOSPC, EIO, a closed pipe) */
        if (rc != 0 || stopped) { /* let the reader run out: hand every buffer back */
            pthread_mutex_lock(&rg.mu);
            for (int i = 0; i < rg.nbuf; i++)
                rg.slot[i].ready = rg.slot[i].filled = 0;
            pthread_cond_broadcast(&rg.cv);
            pthread_mutex_unlock(&rg.mu);
            close(rg.fd); /* read() fails from here on */
        }
        if (rc == 0 && !stopped) { /* (after a failure or a signal the threads are left to the process exit) */
            pthread_join(reader, NULL);
            pthread_join(locker, NULL);
            close(rg.fd);
        }
    }
    const double t_done = now_ms();
    if (timing)
        fprintf(stderr, "timing: runtime init %.1f ms, decode %.1f ms (page-locking, on its own thread: %.1f ms; main thread: %d pushes %.1f ms, "
                        "waiting for a read + locked buffer %.1f ms, formatting + writing %.1f ms, finish %.1f ms), total %.1f ms\n",
                t_init - t_start, t_done - t_init, rg.t_reg, n_push, t_push, t_wait_ring, t_flush, t_finish, t_done - t_start);

    adsb_stats st;
    if (adsb_get_stats(dec, &st) == 0)
        print_stats(&st);
    adsb_format_report rep;
    if (converted && adsb_get_format_report(dec, &rep) == 0 && rep.inexact + rep.clamped > 0)
        fprintf(stderr, "%llu of %llu samples are not %s values (%llu clamped): is -t right?\n", (unsigned long long)(rep.inexact + rep.clamped),
                (unsigned long long)rep.converted, o->stype == ADSB_FMT_INT16_REAL ? "INT16_REAL" : "FLOAT32_REAL", (unsigned long long)rep.clamped);
    if (iq && o->qtype == ADSB_FMT_FLOAT32_IQ && adsb_get_format_report(dec, &rep) == 0 && rep.inexact + rep.clamped > 0)
        fprintf(stderr, "%llu of %llu float scalars were rounded to the int16 grid (%llu clamped): expected of a float32 IQ capture\n",
                (unsigned long long)(rep.inexact + rep.clamped), (unsigned long long)rep.converted, (unsigned long long)rep.clamped);
    cli_exit(rc);
}
