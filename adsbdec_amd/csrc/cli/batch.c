/* batch.c -- the runs over several GPUs or several captures: -G (the library's multi-GPU driver), -B (its batch calls) and
 * -B -E (one batch call of a flush handle). */
#include "cli.h"

static adsb_multi *multi_create(const adsb_config *cfg, int ndev, const int *devs)
{
    adsb_multi *m = adsb_multi_create(cfg, ndev, devs);
    if (!m)
        fprintf(stderr, "adsb_multi_create() failed: %s\n", adsb_multi_last_error(NULL));
    return m;
}

/* The driver cuts FILES into slices (every device preads its own): what the reference accepts beyond that goes the way the
 * one-device run goes it -- a single -f that is a pipe, a FIFO or a device node is streamed through one device (the first
 * one listed), a single -f that cannot be opened ends the run silently with an empty table (air.c:225-228), same bytes on
 * stdout and stderr either way. */
int multi_takes(const struct cli_options *o)
{
    struct stat sb;
    return o->nfiles > 1 || (stat(o->files[0], &sb) == 0 && S_ISREG(sb.st_mode) && access(o->files[0], R_OK) == 0);
}

/* -G: one file: sharded over the devices, same bytes as the one-device run.  Several: one capture per device, packets into
 * <file>.<format>. */
int run_multi(struct cli_options *o)
{
    const int timing = cli_timing(), outformat = o->outformat;
    const adsb_config cfg = cli_config(o);
    restrict_visible_devices(o->devs, o->ndev);
    const int peer = cli_wait_peer();
    if (peer != CLI_PEER_GO)
        return peer == CLI_PEER_ENDED ? 0 : 255;
    const double t_start = now_ms();
    adsb_multi *m = multi_create(&cfg, o->ndev, o->devs);
    if (!m)
        return 255;
    const double t_init = now_ms();
    int rc = 0;
    if (o->nfiles == 1) {
        const adsb_frame *fr = NULL;
        const long n = adsb_multi_decode_file(m, o->files[0], &fr);
        adsb_stats st;
        if (n < 0) {
            fprintf(stderr, "adsb_multi_decode_file() failed: %s\n", adsb_multi_last_error(m));
            rc = 255;
        } else {
            if (write_frames(&out_sink, fr, n, outformat) != 0)
                rc = 1;
            if (sink_close(&out_sink) != 0)
                rc = 1;
            if (timing) {
                adsb_multi_info inf;
                adsb_multi_get_info(m, &inf);
                fprintf(stderr, "timing: runtime init %.1f ms, decode %.1f ms (%d shards, slowest worker %.1f ms, stitch + gather %.0f us%s), total %.1f ms\n",
                        t_init - t_start, now_ms() - t_init, inf.shards, inf.workers_ms, inf.serial_us,
                        inf.fallback ? ", FELL BACK to one device" : "", now_ms() - t_start);
            }
            if (adsb_multi_get_stats(m, &st) == 0)
                print_stats(&st);
        }
    } else {
        adsb_multi_set_long_streams(m, 1); /* one capture per device: ordinary handles, files of any length */
        if (adsb_multi_decode_streams_file(m, o->nfiles, (const char *const *)o->files) != 0) {
            fprintf(stderr, "adsb_multi_decode_streams_file() failed: %s\n", adsb_multi_last_error(m));
            rc = 255;
        }
        for (int k = 0; k < o->nfiles && rc == 0; k++) {
            const adsb_frame *fr = NULL;
            adsb_stats st;
            const long n = adsb_multi_stream_frames(m, k, &fr);
            const int have_st = adsb_multi_stream_stats(m, k, &st) == 0;
            rc = write_capture_file(o->files[k], fr, n, outformat, have_st ? &st : NULL, 0);
        }
        if (timing)
            fprintf(stderr, "timing: runtime init %.1f ms, decode %.1f ms, total %.1f ms\n", t_init - t_start, now_ms() - t_init,
                    now_ms() - t_start);
    }
    cli_exit(rc);
}

/* -B: the paths of a list file, one per line, empty lines skipped.  NULL (with a message) when it cannot be read. */
static char **read_list(const char *listfile, size_t *count)
{
    FILE *f = fopen(listfile, "r");
    if (!f) {
        fprintf(stderr, "%s: cannot read the list of captures: %s\n", listfile, strerror(errno));
        return NULL;
    }
    char **paths = NULL, *line = NULL;
    size_t n = 0, cap = 0, len = 0;
    ssize_t got;
    while ((got = getline(&line, &len, f)) >= 0) {
        while (got > 0 && (line[got - 1] == '\n' || line[got - 1] == '\r'))
            line[--got] = 0;
        if (got == 0)
            continue;
        char **grown = paths;
        if (n == cap && (grown = (char **)realloc(paths, (cap ? 2 * cap : 256) * sizeof *paths)) != NULL) {
            cap = cap ? 2 * cap : 256;
            paths = grown;
        }
        if (!grown || !(paths[n] = strdup(line))) {
            fprintf(stderr, "%s: out of memory for the list of captures\n", listfile);
            while (n > 0)
                free(paths[--n]);
            free(paths);
            free(line);
            fclose(f);
            return NULL;
        }
        n++;
    }
    free(line);
    fclose(f);
    if (!paths) /* (an empty list: nothing to decode, and no error) */
        paths = (char **)calloc(1, sizeof *paths);
    *count = n;
    return paths;
}

/* -B -E: the captures of the list, read whole into memory, through ONE batch call of a flush handle on one GPU (adsb_set_flush +
 * adsb_decode_batch_host / _host_packed); packets and tables go where -B puts them.  The multi-GPU driver has no flush. */
static int run_batch_flush(const adsb_config *cfg, char **paths, size_t n_captures, int packed, int outformat)
{
    void **buf = (void **)calloc(n_captures + 1, sizeof *buf);
    size_t *n = (size_t *)calloc(n_captures + 1, sizeof *n);
    uint64_t *first = (uint64_t *)calloc(n_captures + 1, sizeof *first);
    adsb_stats *st = (adsb_stats *)calloc(n_captures + 1, sizeof *st);
    if (!buf || !n || !first || !st) {
        fprintf(stderr, "out of memory for the results of %zu captures\n", n_captures);
        return 255;
    }
    for (size_t k = 0; k < n_captures; k++) {
        struct stat sb;
        const int fd = open(paths[k], O_RDONLY);
        if (fd < 0 || fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) {
            fprintf(stderr, "%s: cannot read the capture: %s\n", paths[k], fd < 0 ? strerror(errno) : "not a regular file");
            return 255;
        }
        const size_t bytes = (size_t)sb.st_size;
        buf[k] = malloc(bytes ? bytes : 1);
        if (!buf[k]) {
            fprintf(stderr, "%s: out of memory for %zu bytes\n", paths[k], bytes);
            return 255;
        }
        const size_t got = read_full(fd, buf[k], bytes);
        close(fd);
        n[k] = packed ? got / 12 * 8 : got / 2; /* (a trailing odd byte, or partial group, is not decoded: as with -f) */
    }
    adsb_decoder *dec = cli_create(cfg);
    if (!dec)
        return 255;
    const adsb_frame *fr = NULL;
    int rc = 0;
    if (adsb_set_flush(dec, 1) != 0 ||
        (packed ? adsb_decode_batch_host_packed(dec, n_captures, (const void *const *)buf, n, &fr, first, st)
                : adsb_decode_batch_host(dec, n_captures, (const uint16_t *const *)buf, n, &fr, first, st)) < 0) {
        fprintf(stderr, "the batch decode failed: %s\n", adsb_last_error(dec));
        rc = 255;
    }
    for (size_t k = 0; k < n_captures && rc == 0; k++) /* capture by capture: packets into <capture>.<format>, its line and table */
        rc = write_capture_file(paths[k], fr + first[k], (long)(first[k + 1] - first[k]), outformat, &st[k], 1);
    cli_exit(rc);
}

/* -B on the GPUs of -G or the one of -d: ONE start of the runtime, the library's batch calls (adsb_multi_decode_batch_files) */
static int run_batch_multi(const adsb_config *cfg, const int *devs, int ndev, char **paths, size_t n_captures, int packed, int outformat)
{
    const double t_start = now_ms();
    adsb_multi *m = multi_create(cfg, ndev, devs);
    if (!m)
        return 255;
    const double t_init = now_ms();
    int rc = 0;
    const adsb_frame *fr = NULL;
    uint64_t *first = (uint64_t *)calloc(n_captures + 1, sizeof *first);
    adsb_stats *st = (adsb_stats *)calloc(n_captures + 1, sizeof *st);
    if (!first || !st) {
        fprintf(stderr, "out of memory for the results of %zu captures\n", n_captures);
        rc = 255;
    } else if (adsb_multi_decode_batch_files(m, n_captures, (const char *const *)paths, packed, &fr, first, st) < 0) {
        fprintf(stderr, "adsb_multi_decode_batch_files() failed: %s\n", adsb_multi_last_error(m));
        rc = 255;
    }
    const double t_decoded = now_ms();
    for (size_t k = 0; k < n_captures && rc == 0; k++) /* capture by capture: packets into <capture>.<format>, its line and table */
        rc = write_capture_file(paths[k], fr + first[k], (long)(first[k + 1] - first[k]), outformat, &st[k], 1);
    if (cli_timing()) {
        adsb_multi_info inf;
        adsb_multi_get_info(m, &inf);
        fprintf(stderr, "timing: runtime init %.1f ms, decode of %zu captures %.1f ms (%d workers, slowest %.1f ms), writing %.1f ms, total %.1f ms\n",
                t_init - t_start, n_captures, t_decoded - t_init, inf.shards, inf.workers_ms, now_ms() - t_decoded, now_ms() - t_start);
    }
    cli_exit(rc);
}

/* -B: a batch of captures, one path per line of the list */
int run_batch(struct cli_options *o)
{
    size_t n_captures = 0;
    char **paths = read_list(o->listfile, &n_captures);
    if (!paths)
        return 255;
    install_signals();
    if (o->ndev == 0) {
        o->devs[0] = o->device >= 0 ? o->device : 0;
        o->ndev = 1;
    }
    restrict_visible_devices(o->devs, o->ndev);
    adsb_config cfg = cli_config(o);
    if (o->flush) {
        cfg.device = o->devs[0]; /* (restrict_visible_devices has renumbered it where it narrowed the runtime's view) */
        return run_batch_flush(&cfg, paths, n_captures, o->packed, o->outformat);
    }
    return run_batch_multi(&cfg, o->devs, o->ndev, paths, n_captures, o->packed, o->outformat);
}

