/* level.c -- -L: the level report of the file's power samples on stdout, and -L -I: the levels over time; nothing is decoded. */
#include <hip/hip_runtime_api.h> /* the capture and the envelope in device buffers of this program's own */

#include "cli.h"

static double bin_db(unsigned k, int *zero)
{
    /* the lower edge of bin k = (e, f) is 2^(e - 127) (1 + f / 8), a subnormal bin's 2^-126 f / 8: 10 log10 of it */
    static const double m_db[8] = {0.0, 0.51152522447381288, 0.96910013008056415, 1.3830269816628146, 1.7609125905568124,
                                   2.1085336531489318, 2.4303804868629444, 2.7300127206373764};
    static const double f_db[8] = {0.0, -9.0308998699194358, -6.0205999132796242, -4.2596873227228116, -3.0102999566398121,
                                   -2.0411998265592479, -1.2493873660829995, -0.57991946977686754};
    const int e = (int)(k >> 3), f = (int)(k & 7);
    *zero = k == 0;
    return e ? 3.0102999566398121 * (e - 127) + m_db[f] : 3.0102999566398121 * -126 + f_db[f];
}

static unsigned bin_of_quantile(const adsb_level_report *r, double q)
{
    uint64_t total = 0, run = 0;
    for (unsigned k = 0; k < 2048; k++)
        total += r->hist[k];
    const double t = q * (double)total;
    uint64_t need = (uint64_t)t;
    if ((double)need < t)
        need++;
    if (need == 0)
        need = 1;
    for (unsigned k = 0; k < 2048; k++)
        if ((run += r->hist[k]) >= need)
            return k;
    return 0;
}

static void print_db(const char *name, unsigned k, const char *end)
{
    int zero;
    const double db = bin_db(k, &zero);
    if (zero)
        printf("%s -inf dB%s", name, end);
    else if (k >= 2040)
        printf("%s %s%s", name, k == 2040 ? "inf dB" : "nan", end);
    else
        printf("%s %.2f dB%s", name, db, end);
}

/* a report's median, 99.9th percentile and peak bin in dB of raw power units (not dBFS: nobody has measured the front end's
 * gain), each followed by a blank and the last one by `end` */
static void print_summary(const adsb_level_report *rep, const char *end)
{
    unsigned peak = 0, any = 0;
    for (unsigned k = 0; k < 2048; k++)
        if (rep->hist[k])
            peak = k, any = 1;
    if (any) {
        print_db("median", bin_of_quantile(rep, 0.5), " ");
        print_db("p99.9", bin_of_quantile(rep, 0.999), " ");
        print_db("peak", peak, end);
    } else {
        printf("median none p99.9 none peak none%s", end);
    }
}

/* the report as -L prints it: the counters, a line per non-empty bin, the summary */
static void print_level_report(const adsb_level_report *rep)
{
    printf("samples %llu negative %llu rail_lo %llu rail_hi %llu over %llu\n", (unsigned long long)rep->samples, (unsigned long long)rep->negative,
           (unsigned long long)rep->rail_lo, (unsigned long long)rep->rail_hi, (unsigned long long)rep->over);
    for (unsigned k = 0; k < 2048; k++) {
        if (!rep->hist[k])
            continue;
        union { uint32_t u; float f; } edge;
        edge.u = k << 20;
        if (k < 2040)
            printf("bin %u %.9g %llu\n", k, (double)edge.f, (unsigned long long)rep->hist[k]);
        else
            printf("bin %u %s %llu\n", k, k == 2040 ? "inf" : "nan", (unsigned long long)rep->hist[k]);
    }
    print_summary(rep, "\n");
}

/* -L.  The whole file is ONE capture in ONE call (the report of a real capture needs every pair's six predecessors, and only the
 * uint16 flavour has a window call: -I, run_level_windows below): kind 0 uint16 (adsb_level_host, through the handle's buffers),
 * 1 -t 1 | 3, 2 -p, 3 -q, 4 -w (a device buffer of the program's own). */
int run_level(const struct cli_options *o)
{
    const int kind = o->converted ? 1 : o->packed ? 2 : o->iq ? 3 : o->power ? 4 : 0, fmt = o->iq ? (int)o->qtype : (int)o->stype;
    int device = o->device;
    const int fd = open(o->filename, O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) {
        fprintf(stderr, "%s: cannot read as a regular file: %s\n", o->filename, fd < 0 ? strerror(errno) : "-L takes the whole file in one call");
        return 255;
    }
    adsb_decoder *dec = cli_create_on(&device);
    if (!dec)
        return 255;
    const size_t elem = kind == 0 ? 2 : kind == 1 ? adsb_format_bytes(fmt, 1) : kind == 3 ? adsb_iq_bytes(fmt, 1) : kind == 4 ? sizeof(float) : 0;
    void *buf = malloc((size_t)sb.st_size + 16), *d_in = NULL;
    adsb_level_report *rep = (adsb_level_report *)malloc(sizeof *rep);
    if (!buf || !rep) {
        fprintf(stderr, "out of memory for the file's %lld bytes\n", (long long)sb.st_size);
        return 255;
    }
    const size_t bytes = read_full(fd, buf, (size_t)sb.st_size);
    const size_t n = kind == 2 ? bytes / 12 * 8 : bytes / elem, used = kind == 2 ? bytes / 12 * 12 : n * elem;
    const size_t real_tail = kind <= 1 ? (n % 4) * elem : 0; /* (the reference reads four samples at a time) */
    if (bytes - used + real_tail)
        fprintf(stderr, "%zu trailing bytes ignored (%s)\n", bytes - used + real_tail,
                kind == 2 ? "not a whole 12-byte group of packed samples" : kind <= 1 ? "the reference reads four samples at a time" : "not a whole sample");
    long got;
    const char *call = "adsb_level_host";
    /* -U: the envelope too, into a device array of this program's (a real capture: from HBM as well, where the envelope has to be) */
    const int gate = o->burst.factor > 0;
    const uint64_t m_guess = kind <= 2 ? 2 * (uint64_t)(n / 4) : n;
    const size_t env_cap = gate ? (size_t)((m_guess + 27) / 28) : 0;
    float *d_env = NULL;
    if (kind == 0 && !gate) {
        got = adsb_level_host(dec, (const uint16_t *)buf, n, rep, NULL, 0);
    } else {
        if (hipSetDevice(device < 0 ? 0 : device) != hipSuccess || (used && hipMalloc(&d_in, used) != hipSuccess) ||
            (used && hipMemcpy(d_in, buf, used, hipMemcpyHostToDevice) != hipSuccess)) {
            fprintf(stderr, "cannot bring the file's %zu bytes to the device\n", used);
            return 255;
        }
        if (env_cap && hipMalloc((void **)&d_env, env_cap * sizeof(float)) != hipSuccess) {
            fprintf(stderr, "cannot allocate the envelope's %zu floats on the device\n", env_cap);
            return 255;
        }
        if (kind == 0)
            call = "adsb_level_device", got = adsb_level_device(dec, d_in, n, rep, d_env, env_cap);
        else if (kind == 1)
            call = "adsb_level_device_as", got = adsb_level_device_as(dec, fmt, d_in, n, rep, d_env, env_cap);
        else if (kind == 2)
            call = "adsb_level_device_packed", got = adsb_level_device_packed(dec, d_in, n, rep, d_env, env_cap);
        else if (kind == 3)
            call = "adsb_level_device_iq", got = adsb_level_device_iq(dec, fmt, d_in, n, rep, d_env, env_cap);
        else
            call = "adsb_level_device_power", got = adsb_level_device_power(dec, d_in, n, rep, d_env, env_cap);
    }
    if (got < 0) {
        fprintf(stderr, "%s() failed: %s\n", call, adsb_last_error(dec));
        return 255;
    }
    print_level_report(rep);
    if (gate) {
        const int rc = level_bursts(dec, o, rep, d_env, (uint64_t)got, kind, fmt, d_in, n, used);
        if (rc) {
            fflush(stdout);
            return rc;
        }
    }
    fflush(stdout);
    cli_exit(0);
}

/* -L -I ms: the levels over time.  The file -- a FIFO will do -- is read in pieces of LEVEL_PIECE power samples at most, each behind the
 * last 16 samples of the piece before it, so that every power sample has its six older pairs; a piece is ONE adsb_level_windows_host
 * call over windows of `ms` milliseconds (10 000 power samples each, rounded down to a multiple of 28).  A line per window, then -L's
 * own report of their sum (adsb_level_add). */
#define LEVEL_PIECE ((uint64_t)28 * 299593) /* about 16 Mi samples */
#define LEVEL_PIECE_WINDOWS 1024            /* one launch (adsbdec_amd.h) */
#define LEVEL_OVERLAP 16
int run_level_windows(const struct cli_options *o)
{
    const double ms = o->interval_ms, per_ms = 10000.0; /* power samples: 20 MS/s real, a power sample per pair */
    int device = o->device;
    const uint64_t win = ms * per_ms >= (double)LEVEL_PIECE ? LEVEL_PIECE : (uint64_t)(ms * per_ms) / 28 * 28;
    if (win == 0) {
        fprintf(stderr, "-I %g: a window holds at least 28 power samples (0.0028 ms)\n", ms);
        return 1;
    }
    if (ms * per_ms > (double)LEVEL_PIECE)
        fprintf(stderr, "-I %g: windows of %llu power samples (%.4f ms), the most this program reads at once\n", ms, (unsigned long long)win,
                (double)win / per_ms);
    const int fd = open(o->filename, O_RDONLY);
    if (fd < 0) {
        fprintf(stderr, "%s: cannot read: %s\n", o->filename, strerror(errno));
        return 255;
    }
    adsb_decoder *dec = cli_create_on(&device);
    if (!dec)
        return 255;
    uint64_t k_max = LEVEL_PIECE / win;
    if (k_max > LEVEL_PIECE_WINDOWS)
        k_max = LEVEL_PIECE_WINDOWS;
    const char *few = getenv("ADSB_CLI_LEVEL_PIECE"); /* (for tests: the most windows of a piece, so that a small file takes several) */
    if (few && atoi(few) > 0 && (uint64_t)atoi(few) < k_max)
        k_max = (uint64_t)atoi(few);
    const uint64_t piece = k_max * win; /* power samples */
    uint16_t *buf = (uint16_t *)malloc((LEVEL_OVERLAP + 2 * piece) * sizeof(uint16_t) + 1);
    uint64_t *edges = (uint64_t *)malloc((k_max + 1) * sizeof(uint64_t));
    adsb_level_report *rep = (adsb_level_report *)malloc((k_max + 1) * sizeof *rep), *sum = rep ? rep + k_max : NULL;
    if (!buf || !edges || !rep) {
        fprintf(stderr, "out of memory for pieces of %llu samples\n", (unsigned long long)(2 * piece));
        return 255;
    }
    memset(sum, 0, sizeof *sum);
    uint64_t done = 0; /* power samples reported: a multiple of win */
    for (;;) {
        const size_t bytes = read_full(fd, buf + LEVEL_OVERLAP, 2 * piece * sizeof(uint16_t));
        const size_t n_new = bytes / sizeof(uint16_t);
        const uint64_t m_new = 2 * (uint64_t)(n_new / 4);
        const int last = bytes < 2 * piece * sizeof(uint16_t);
        if (last && bytes - 2 * m_new * sizeof(uint16_t))
            fprintf(stderr, "%zu trailing bytes ignored (the reference reads four samples at a time)\n", bytes - (size_t)(2 * m_new) * sizeof(uint16_t));
        size_t k = 0;
        for (edges[0] = done; edges[k] < done + m_new; k++)
            edges[k + 1] = edges[k] + win < done + m_new ? edges[k] + win : done + m_new;
        if (k) {
            const int head = done ? LEVEL_OVERLAP : 0; /* (the stream's start has nothing in front of it) */
            if (adsb_level_windows_host(dec, buf + LEVEL_OVERLAP - head, 2 * done - head, n_new + head, k, edges, rep, NULL, 0) < 0) {
                fprintf(stderr, "adsb_level_windows_host() failed: %s\n", adsb_last_error(dec));
                return 255;
            }
        }
        for (size_t i = 0; i < k; i++) {
            const adsb_level_report *r = &rep[i];
            printf("t %.6f s ", (double)edges[i] / (per_ms * 1000.0));
            print_summary(r, " ");
            printf("rail_lo %llu rail_hi %llu over %llu\n", (unsigned long long)r->rail_lo, (unsigned long long)r->rail_hi, (unsigned long long)r->over);
            adsb_level_add(sum, r);
        }
        if (last)
            break;
        done += m_new;
        memcpy(buf, buf + 2 * piece, LEVEL_OVERLAP * sizeof(uint16_t)); /* the piece's last 16 samples, in front of the next */
    }
    print_level_report(sum);
    fflush(stdout);
    cli_exit(0);
}
