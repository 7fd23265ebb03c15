/* common.c -- what every mode of the host program uses: signals, the device narrowing, the handle, the sink, the packets'
 * and the table's way out, the exit. */
#include <signal.h>
#include <time.h>

#include "cli.h"

sink out_sink;

/* main.c:91-99: SIGINT / SIGTERM / SIGQUIT end the run in an orderly way -- the reference's handlerExit sets do_exit, the
 * writer loop ends, main prints the Try/Ok table and returns runOutput()'s 0 -- and SIGPIPE is ignored, so that a closed
 * stdout or peer shows up as a failed write, not as death by signal.  Here: the handler sets a flag (no SA_RESTART: a
 * blocking accept / connect / read returns), the push loop stops at the next buffer, what has been decoded is finished,
 * written and counted, the table is printed, exit status 0. */
volatile int stop_requested;
static void on_stop_signal(int sig)
{
    (void)sig;
    stop_requested = 1;
}
void install_signals(void)
{
    struct sigaction sa;
    memset(&sa, 0, sizeof sa);
    sigemptyset(&sa.sa_mask);
    sa.sa_handler = on_stop_signal;
    sigaction(SIGTERM, &sa, NULL);
    sigaction(SIGQUIT, &sa, NULL);
    sigaction(SIGINT, &sa, NULL);
    sa.sa_handler = SIG_IGN;
    sigaction(SIGPIPE, &sa, NULL);
}

double now_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
}

int cli_timing(void)
{
    const char *t = getenv("ADSB_CLI_TIMING");
    return t ? (atoi(t) > 1 ? 2 : 1) : 0;
}

/* No adsb_destroy / unregister / free in front of it: the process ends here, and tearing the GPU runtime down cleanly costs
 * tens of milliseconds that an offline run has no use for. */
void cli_exit(int rc)
{
    fflush(stderr);
    if (getenv("ADSB_CLI_CLEAN_EXIT")) /* (a profiler's knob: rocprofv3 writes its trace from an exit handler) */
        exit(rc);
    _exit(rc);
}

/* read() until `want` bytes are in or the file ends */
size_t read_full(int fd, void *buf, size_t want)
{
    size_t got = 0;
    while (got < want) {
        const ssize_t k = read(fd, (char *)buf + got, want - got);
        if (k <= 0)
            break;
        got += (size_t)k;
    }
    return got;
}

/* Narrow the runtime's view to the devices in use, BEFORE its first call (it initialises every device it sees), and
 * renumber devs[] to the ordinals the runtime will then hand out.  A caller's own ROCR_VISIBLE_DEVICES is left alone. */
void restrict_visible_devices(int *devs, int n)
{
    if (getenv("ROCR_VISIBLE_DEVICES") || getenv("HIP_VISIBLE_DEVICES") || getenv("ADSB_CLI_ALL_DEVICES"))
        return;
    int uniq[MAX_GPUS], nu = 0;
    char list[8 * MAX_GPUS] = "";
    for (int i = 0; i < n; i++) {
        int at = -1;
        for (int k = 0; k < nu; k++)
            if (uniq[k] == devs[i])
                at = k;
        if (at < 0) {
            at = nu;
            uniq[nu++] = devs[i];
            snprintf(list + strlen(list), sizeof list - strlen(list), "%s%d", nu > 1 ? "," : "", devs[i]);
        }
        devs[i] = at;
    }
    setenv("ROCR_VISIBLE_DEVICES", list, 1);
}

/* One device is all the run uses, that of -d or the first: do not start the others.  *device stays -1 without -d (the handle
 * then takes the current device, which is the first). */
void cli_one_device(int *device)
{
    int first = 0;
    restrict_visible_devices(*device >= 0 ? device : &first, 1);
}

/* the config of a run that decodes; .device (and .warm_start) are the caller's */
adsb_config cli_config(const struct cli_options *o)
{
    adsb_config cfg;
    adsb_config_default(&cfg);
    cfg.df18 = o->df18;
    cfg.fix_1bit = o->fix1;
    cfg.collect_stats = 1; /* the reference always prints Try/Ok */
    return cfg;
}

/* NULL behind a message: the caller returns 255, runOutput() == -1 -> exit status 255 (main.c:101-105) */
adsb_decoder *cli_create(const adsb_config *cfg)
{
    adsb_decoder *dec = adsb_create(cfg);
    if (!dec)
        fprintf(stderr, "adsb_create() failed: %s\n", adsb_last_error(NULL));
    return dec;
}

/* the handle of a run that decodes nothing (-W, -L): the default config, on *device as cli_one_device leaves it */
adsb_decoder *cli_create_on(int *device)
{
    adsb_config cfg;
    adsb_config_default(&cfg);
    cli_one_device(device);
    cfg.device = *device;
    return cli_create(&cfg);
}

void cli_open_sink(const struct cli_options *o)
{
    sink_init(&out_sink, o->outmode, o->rawaddr);
    out_sink.stop = &stop_requested;
    if (getenv("ADSB_CLI_RETRY_S")) /* (a test's knob: the reference waits 3 s between attempts, output.c:282) */
        out_sink.retry_s = (unsigned)atoi(getenv("ADSB_CLI_RETRY_S"));
}

/* -s / -l: the peer first (output.c:277-285: no peer, no packets).  ENDED: told to end before a peer came -- nothing decoded,
 * the table (all zero) is on stderr, status 0 (main.c:101-105).  FAILED: an unusable address, runOutput() == -1
 * (output.c:278-279), status 255. */
int cli_wait_peer(void)
{
    const int prc = sink_wait_peer(&out_sink);
    if (prc == 2) {
        adsb_stats z;
        memset(&z, 0, sizeof z);
        print_stats(&z);
        return CLI_PEER_ENDED;
    }
    return prc != 0 ? CLI_PEER_FAILED : CLI_PEER_GO;
}

/* Packets leave in batches of up to 64 KiB: one fwrite / send per batch. */
int write_frames(sink *out, const adsb_frame *fr, long n, int outformat)
{
    static char batch[65536 + 256];
    size_t fill = 0;
    unsigned long packets = 0;
    for (long i = 0; i < n; i++) {
        fill += (size_t)adsb_format_frame(&fr[i], outformat, batch + fill);
        packets++;
        if (fill >= 65536 || i + 1 == n) {
            const int rc = sink_write(out, batch, fill, packets);
            if (rc < 0)
                return -1;
            fill = 0, packets = 0; /* (rc == 1: the peer went away and the batch with it, output.c:321-327) */
        }
    }
    return 0;
}

void print_stats(const adsb_stats *st) /* valid.c:84-100 */
{
    unsigned long long tot = st->ok[0] + st->ok[1] + st->ok[2];
    fprintf(stderr, "\t%10d\t%10d\t%10d\n", 11, 17, 18);
    fprintf(stderr, "Try :\t%10llu\t%10llu\t%10llu\n", (unsigned long long)st->try_[0], (unsigned long long)st->try_[1],
            (unsigned long long)st->try_[2]);
    fprintf(stderr, "Ok :\t%10llu\t%10llu\t%10llu\n", (unsigned long long)st->ok[0], (unsigned long long)st->ok[1],
            (unsigned long long)st->ok[2]);
    fprintf(stderr, "Total :\t%10llu\n", tot); /* tot_fi is uninitialised there */
}

/* One capture's n packets (n < 0: it has none to give) into <path_base>.avr | .mlat | .beast, then its line and, where there
 * is one, its table on stderr.  0, or 1 behind a message.  check_name: a name that does not fit is refused by name (-B);
 * several -f with -G have never looked, and a name cut short there simply cannot be written. */
int write_capture_file(const char *path_base, const adsb_frame *fr, long n, int outformat, const adsb_stats *st, int check_name)
{
    static const char *ext[3] = {"avr", "mlat", "beast"};
    char path[4096], pkt[256];
    if ((size_t)snprintf(path, sizeof path, "%s.%s", path_base, ext[outformat]) >= sizeof path && check_name) {
        fprintf(stderr, "%s: the name of its .%s file is longer than %zu bytes\n", path_base, ext[outformat], sizeof path - 1);
        return 1;
    }
    FILE *out = n >= 0 ? fopen(path, "wb") : NULL;
    int bad = !out;
    for (long i = 0; !bad && i < n; i++) {
        const int len = adsb_format_frame(&fr[i], outformat, pkt);
        bad = fwrite(pkt, 1, (size_t)len, out) != (size_t)len;
    }
    if (bad || fclose(out) != 0) {
        fprintf(stderr, "%s: cannot write\n", path);
        return 1;
    }
    fprintf(stderr, "== %s: %ld frames -> %s\n", path_base, n, path);
    if (st)
        print_stats(st);
    return 0;
}
