/* cli.h -- what the files of the host program share: the options record, the helpers every mode uses (common.c) and the
 * modes' entry points.  Internal to csrc/cli/; the manual is the comment at the head of adsbdec_amd_cli.c. */
#ifndef ADSBDEC_AMD_CLI_H
#define ADSBDEC_AMD_CLI_H
#include <errno.h>
#include <fcntl.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>

#include "adsbdec_amd.h"
#include "sink.h"

#define MAX_GPUS 64
#define MAX_FILES 64

struct burst_opts { /* -U: factor 0 = no gate */
    double factor;
    uint32_t lead, hang;
};

struct record_opts { /* -S: factor 0 = malformed.  absolute: the argument began with @ and factor is the threshold itself */
    double factor;
    int absolute;
    uint32_t lead, hang;
    uint64_t piece; /* runs read per slice */
};

/* The command line as cli_parse leaves it.  A malformed -t, -q, -I or -U is remembered here (stype / qtype -1, interval_ms 0,
 * burst.factor 0) beside the text the refusal echoes; cli_refuse turns it away. */
struct cli_options {
    const char *filename; /* the last -f */
    char *files[MAX_FILES];
    int nfiles;
    const char *listfile;    /* -B */
    const char *export_path; /* -W */
    int devs[MAX_GPUS], ndev; /* -G */
    int device;               /* -d, or -1 */
    int outformat, df18, fix1, packed, power, level, flush;
    const char *burst_arg; /* -U: -L's gate, factor[,lead[,hang]] */
    struct burst_opts burst;
    const char *archive_out; /* -K: keep only the bursts of -L -U, as a burst archive */
    const char *pack_out;    /* -P: ... of a real capture, packed to 12 bits (archive kind 12) */
    int archive_in;          /* -k: the file of -f is a burst archive */
    const char *record_arg;  /* -S: gate a stream of any length, factor[,lead[,hang[,piece]]] */
    struct record_opts record;
    const char *record_out;  /* -O: ... and keep its bursts as a burst archive */
    const char *interval_arg; /* -I: -L's windows, in milliseconds */
    double interval_ms;
    long stype; /* -t: ADSB_FMT_RAW without it */
    const char *stype_arg;
    long qtype; /* -q: ADSB_FMT_INT16_IQ / ADSB_FMT_FLOAT32_IQ / ADSB_FMT_INT8_IQ */
    const char *qtype_arg;
    int outmode; /* SINK_STDOUT unless -s / -l */
    const char *rawaddr;
    int converted, iq; /* -t 1 | 3; any -q */
};

/* options.c: 0, or the exit status behind the usage text or a refusal on stderr.  Neither touches a file or the runtime. */
int cli_parse(int argc, char **argv, struct cli_options *o);
int cli_refuse(const struct cli_options *o);

/* common.c */
extern sink out_sink;              /* stdout unless -s / -l */
extern volatile int stop_requested; /* SIGINT / SIGTERM / SIGQUIT */
void install_signals(void);
double now_ms(void);
int cli_timing(void); /* ADSB_CLI_TIMING: 0, 1, or 2 (a line per push too) */
void cli_exit(int rc) __attribute__((noreturn));
size_t read_full(int fd, void *buf, size_t want);
void restrict_visible_devices(int *devs, int n);
void cli_one_device(int *device);
adsb_config cli_config(const struct cli_options *o);
adsb_decoder *cli_create(const adsb_config *cfg);
adsb_decoder *cli_create_on(int *device);
void cli_open_sink(const struct cli_options *o);
enum { CLI_PEER_GO = 0, CLI_PEER_ENDED, CLI_PEER_FAILED };
int cli_wait_peer(void);
int write_frames(sink *out, const adsb_frame *fr, long n, int outformat);
void print_stats(const adsb_stats *st);
int write_capture_file(const char *path_base, const adsb_frame *fr, long n, int outformat, const adsb_stats *st, int check_name);

/* the modes: each returns only on a failure (main ends with that status) and leaves through cli_exit otherwise */
int run_stream(const struct cli_options *o);                    /* stream.c: one capture on one GPU */
int multi_takes(const struct cli_options *o);                   /* batch.c: -G */
int run_multi(struct cli_options *o);
int run_batch(struct cli_options *o);                           /* -B, -B -E */
int run_export(const struct cli_options *o);                    /* export.c: -W */
int run_level(const struct cli_options *o);                     /* level.c: -L */
int run_level_windows(const struct cli_options *o);             /* -L -I */
/* bursts.c: -U's gate behind run_level's report, then -K | -P; the capture as run_level has it on the device */
int level_bursts(adsb_decoder *dec, const struct cli_options *o, const adsb_level_report *rep, const float *d_env, uint64_t m,
                 int flavour, int fmt, const void *d_in, size_t n, size_t used);
int run_archive(const struct cli_options *o);                   /* -k */
int run_record(const struct cli_options *o);                    /* record.c: -S [-O] */
#endif
