/*
 * adsbdec_amd_cli.c -- host program in C for the offline "-f" path, calling the
 * HIP library through the C-ABI of include/adsbdec_amd.h.
 *
 * Mirrors the reference's command line for this path (main.c:60-89):
 *     -f filename   input file (air.c:217-246 fileInput)
 *     -a            also decode DF18 (sets `df`, main.c:76-78 / demod.c:26)
 *     -m            AVR-MLAT output (outformat 1, main.c:79-81)
 *     -b            Beast binary output (outformat 2, main.c:82-84)
 *     -g n          accepted and ignored (gain only matters for the live radio)
 *     -x            EXTENSION, not in the reference: repair single-bit errors in DF17/18
 *                   frames (the reference's -e flag is parsed but does nothing and exits
 *                   with the usage text, main.c:40,60,85-87; that behaviour is kept for -e)
 *     -d k          EXTENSION: decode on GPU k of the node (default: the first one)
 *     -p            EXTENSION: the file holds Airspy packed 12-bit samples (adsbdec_amd.h: the format; -p as in
 *                   airspy_rx), unpacked on the GPU.  A trailing partial group (file size % 12 != 0) is not decoded and
 *                   stderr says how many bytes were ignored.  Not with -G (the multi-GPU driver reads uint16 files only).
 *     -t type       EXTENSION: the sample type of the file, numbered as airspy_rx -t numbers them (adsbdec_amd.h: the formats).
 *                   1 (float32 real) and 3 (signed 16-bit real, what adsbdec's README calls "raw signed 16 bits real") are
 *                   converted on the GPU; 4 and 5 are the uint16 code this program reads without -t; 0 and 2 (IQ) and
 *                   anything else are refused.  A trailing partial sample is not decoded and stderr says how many bytes
 *                   were ignored.  A run in which samples were off the format's grid ends with a line on stderr that says
 *                   how many: the sign of a wrong -t.  -t 1 and -t 3 not with -p, -G or -B.
 *     -q type       EXTENSION: the file holds COMPLEX samples at 10 MS/s, numbered as airspy_rx -t numbers them: 2 INT16_IQ (its
 *                   default), 0 FLOAT32_IQ (adsbdec_amd.h: the _iq calls).  Not with -t, -p, -G or -B; a file below 2^31 samples.
 *                   -q 8 is NOT an airspy_rx number: INT8_IQ, interleaved signed bytes I, Q as hackrf_transfer -r writes them (cs8;
 *                   bladeRF and USRP sc8 are the same bytes), decoded as the int16 capture (I << 8, Q << 8) is.  Not with -w or -W
 *                   either.
 *     -w            EXTENSION: the file holds float32 POWER samples at 10 MS/s, little-endian: the reference's ampbuff stream itself
 *                   (adsbdec.h:5), from any front end (adsbdec_amd.h: the _power calls).  Input domain: every sample finite, sign bit
 *                   clear, below 2^29 (no negatives, -0.0, NaN, Inf; subnormals are fine); outside it nothing is promised (-L -w detects it).
 *                   Trailing bytes that do not make a sample are not decoded and stderr says how many.  Not with -t, -q, -p, -G or
 *                   -B; a file below 2^31 samples.
 *     -W out.pw     EXTENSION: EXPORT instead of decoding: write the float32 power samples of the file of -f -- the reference's ampbuff
 *                   (air.c:54-91), what -w reads -- to out.pw, little-endian, and print nothing.  A uint16 file is read in pieces of about
 *                   4 Mi samples, each with 16 samples of overlap in front, through adsb_power_window_host: bounded memory, any length
 *                   below 2^32 samples; a trailing n % 4 samples give no output.  With -q 2 | 0 the file is IQ: one power sample per
 *                   complex sample, pieces without overlap through a device buffer of this program's and adsb_power_device_iq: any
 *                   length.  out.pw is created once the GPU is open; a signal between two pieces ends the program with status 1 and a
 *                   message (out.pw then holds the pieces so far).  Not with -w, -t (python -m adsbdec_amd.sample_formats converts
 *                   such files), -p, -G, -B, -s, -l or several -f.
 *     -L            EXTENSION: REPORT THE LEVELS instead of decoding (adsbdec_amd.h: the adsb_level_* calls): of the power samples -W would
 *                   write -- or, with -p, -t 1 | 3, -q 2 | 0 | 8 or -w, of that input's -- print `samples M negative N rail_lo A rail_hi B
 *                   over C`, a line `bin K lower_edge COUNT` per non-empty bin of the histogram (1/8 octave, 0.75 dB), and the median, the
 *                   99.9th percentile and the peak bin in dB of raw power units (not dBFS: nobody has measured the front end's gain).  The
 *                   whole file is one capture in one call: a real file below 2^32 samples, IQ and power below 2^31.  Not with -G, -B,
 *                   -W, -s, -l or several -f.
 *     -I ms         EXTENSION, with -L on a uint16 file: THE LEVELS OVER TIME (adsb_level_windows_host).  The file, or FIFO, is read in
 *                   pieces of about 16 Mi samples, each behind the last 16 samples of the piece before it; a line `t START s median ..
 *                   p99.9 .. peak .. rail_lo A rail_hi B over C` per window of ms milliseconds (10 000 power samples each, rounded down
 *                   to a multiple of 28), then -L's report of the sum of the windows (a trailing n % 4 samples belong to no window: named
 *                   on stderr, and not on the rails as plain -L has them).  Not with -t, -p, -q or -w.
 *     -U factor[,lead[,hang]]  EXTENSION, with -L: FIND THE BURSTS (adsb_bursts_device).  The level call also writes the envelope, one float
 *                   per 28 power samples, into a device array of this program's; threshold = factor * the median bin's lower edge
 *                   (adsb_level_percentile at 0.5); behind -L's report a line `bursts B threshold T lead L hang H`, then a line per burst
 *                   `FIRST END HOT PEAK`: power samples [FIRST, END), its hot runs, its largest envelope float.  lead and hang (runs of 28
 *                   power samples kept before the first and behind the last hot run) default to 2 and 1468.  WIDENED from the 2 and 4
 *                   first meant: with hang 4 the pipeline fixture (tests/burst_cases.py) loses EVERY planted frame, because a decode call
 *                   keeps the reference's end-of-file horizon -- deqframe runs only once 40 980 power samples are in (air.c:94-99), so a
 *                   piece shorter than that decodes nothing; 1468 runs are 41 104 power samples behind the last hot run.  The values
 *                   rest on that ONE fixture, not on a measurement of live traffic.  Every flavour -L reads; not with -I.
 *                   Pieces that are decoded with -E (a flush handle) need no such length: hang 4 is enough there.
 *     -K out.brs    EXTENSION, with -L -U: KEEP ONLY THE BURSTS (adsb_gather_device).  Behind -L's report and -U's lines the pieces the gate
 *                   found are packed, on the GPU and out of the capture the level call has already read in HBM, into one array -- piece i
 *                   is the capture's own bytes of power samples [28 begin_i, min(28 end_i, M)), each piece from a multiple of 16 bytes on,
 *                   pad bytes zero -- copied back in ONE device-to-host copy and written to out.brs: a burst archive (burst_archive.h;
 *                   adsbdec_amd/burst_archive.py reads and writes the same bytes).  On stderr `kept B bursts, X of Y bytes`.  A uint16 file,
 *                   -q 2 | 0 | 8 or -w.  Not without -L -U; not with -t or -p (their pieces are not in the capture's own bytes), -I (one
 *                   file, one call: bursts are not joined across pieces), -G, -B or -W.
 *     -P out.brs    EXTENSION, with -L -U: KEEP ONLY THE BURSTS OF A REAL CAPTURE, AT 12 BITS (adsb_gather_pack12_*).  What -K does, for
 *                   a uint16 file (the default), -p or -t 3 | 1: the pieces are gathered out of the capture's uint16 twin in HBM -- the
 *                   capture itself, or the scratch its level call has unpacked or converted it into -- and packed while they are copied
 *                   into Airspy packed 12-bit samples, 3 bytes per power sample where -K writes 4; a clipped last piece is completed to
 *                   a whole group of 8 with code 2048.  The archive's kind is 12 (sample_bytes 3); -k decodes it through
 *                   adsb_decode_batch_host_packed.  On stderr `kept B bursts, X of Y bytes`.  A sample above 4095 inside a burst does
 *                   not fit 12 bits: the run says how many there are, writes NO archive and exits with status 255 (-K keeps all 16
 *                   bits).  Not without -L -U; not with -q, -w, -K, -I, -G, -B, -W or -k.
 *     -k            EXTENSION: the file of -f is a BURST ARCHIVE.  Its pieces are decoded by ONE adsb_decode_batch_host* call of the
 *                   archive's kind on a flush handle (a piece is far below the end-of-file horizon, so each is decoded as -E decodes a
 *                   file: as its silent twin); the packets are printed in order with positions in the original capture: g + 28 begin_i
 *                   is exact, the timestamp ts + 28 begin_i is the original's only up to what the frames accepted before the piece had
 *                   jumped (demod.c:99,128,134).  The table is the sum of the pieces' tables.  -a, -m, -b, -x, -s, -l as for a capture; the
 *                   kind comes from the header: not with -t, -p, -q, -w, -E, -G, -B, -L, -W or -K.  A file that is no archive of this
 *                   version, or whose table and payload do not go together, is refused before any GPU call.
 *     -E            EXTENSION: DECODE TO THE LAST SAMPLE (adsb_set_flush).  The reference never scans the last ~41 k power samples of a
 *                   file -- deqframe runs only once 40 980 power samples are buffered (air.c:94-99) and scans idx < len - 1200
 *                   (demod.c:89) -- and a file below 81 960 samples decodes nothing.  With -E the packets and the table are what the
 *                   reference prints for the file followed by 81 960 power samples of silence: every packet of the run without -E, in
 *                   front and unchanged, then those of the file's end.  Every input kind of -f (-p, -t, -q, -w), and -B on one GPU
 *                   (adsb_decode_batch_host* on a flush handle: the captures are read whole into memory).  A real file stays below 2^32
 *                   samples here (a long stream has no flush).  Not with -G (the multi-GPU driver keeps the horizon), -L or -W (which
 *                   decode nothing).
 *     -G n | a,b,c  EXTENSION: shard the file over n GPUs (or over the GPUs listed; an ordinal may repeat) through
 *                   the library's multi-GPU driver (adsb_multi_decode_file): same bytes on stdout and stderr.
 *                   With several -f (one capture each) the captures are decoded side by side, one per GPU, and
 *                   capture k's packets go to <file k>.avr / .mlat / .beast instead of stdout.
 *     -B listfile   EXTENSION: a batch of captures, one path per line of listfile (empty lines are skipped; any number of
 *                   them).  The runtime's start is paid once for all: the captures are decoded through the library's
 *                   batch calls (adsb_multi_decode_batch_files), many short ones per launch, on the GPUs of -G or on the
 *                   one of -d (default: the first one).  Capture k's packets go to <capture k>.avr / .mlat / .beast and
 *                   stderr has, per capture, the line and the table several -f with -G print.  -p is allowed here (every
 *                   capture is then a packed one; a trailing partial group is not decoded).  Not with -f, -s or -l.
 * The GPU runtime initialises every device it can see, which takes longer the more there are: before its first call
 * this program narrows ROCR_VISIBLE_DEVICES to the devices it is going to use (unless the variable is already set).
 *     -s addr[:port]  send the packets to a TCP peer instead of stdout (main.c:65-68; default port 30001)
 *     -l addr[:port]  listen, accept ONE peer and send the packets to it (main.c:69-72; default port 30002); sink.c
 * The live Airspy input and anything else print the usage text and exit 1, like the reference's default: branch
 * (main.c:85-87).
 *
 * Differences from the reference, on purpose (DESIGN.md "CLI"):
 *   - every accepted frame is written: the reference drops frames still queued
 *     when the reader thread hits EOF;
 *   - Beast to stdout is written with its real length (the reference uses strlen()
 *     on a binary buffer).
 * The stderr statistics table has the reference's format (valid.c:84-100).
 * Signals as in main.c:91-99: SIGPIPE ignored; SIGINT / SIGTERM / SIGQUIT stop the pushes, what has been decoded is
 * finished and written, the table is printed, exit status 0.
 */
#include <fcntl.h>
#include <errno.h>
#include <pthread.h>
#include <signal.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/mman.h>
#include <sys/stat.h>
#include <time.h>
#include <unistd.h>

#include <hip/hip_runtime_api.h> /* -W -q: a device buffer of this program's own (three calls) */

#include "adsbdec_amd.h"
#include "burst_archive.h"
#include "sink.h"

/* fileInput (air.c:217-246) reads 2 MiB at a time into one buffer and decodes it before the
 * next read().  Here a reader thread fills a ring of 32 MiB buffers from the moment the
 * program starts -- so the file is being read while the GPU runtime initialises (~0.2 s) --
 * and the main thread hands each filled buffer to adsb_push_async(), which overlaps the
 * host-to-device copy of one buffer with the scan of the previous one. */
#define BUF_SAMPLES (16u * 1024u * 1024u)
#define RING_MAX_BYTES (1024ull * 1024ull * 1024ull)
/* bytes per ring buffer: BUF_SAMPLES samples, as uint16 (32 MiB), packed 12-bit with -p (24 MiB: whole 12-byte groups), or what
 * adsb_format_bytes says for -t 1 / -t 3 */
static size_t buf_bytes = (size_t)BUF_SAMPLES * 2;

typedef struct {
    uint16_t *buf;
    size_t bytes; /* valid bytes once filled */
    int filled;
    int registered;
    int ready;    /* filled, and page-locked if that was asked for: the main thread may push it */
} ring_slot;

typedef struct {
    int fd, nbuf, failed, use_register;
    double t_reg;
    ring_slot *slot;
    pthread_mutex_t mu;
    pthread_cond_t cv;
} ring;

static void *reader_main(void *arg)
{
    ring *r = (ring *)arg;
    const size_t cap = buf_bytes;
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
        size_t got = 0;
        while (s->buf && got < cap) { /* fill the buffer: only the last one of a file is short */
            ssize_t n = read(r->fd, (char *)s->buf + got, cap - got);
            if (n <= 0)
                break;
            got += (size_t)n;
        }
        pthread_mutex_lock(&r->mu);
        s->bytes = got;
        s->filled = 1;
        pthread_cond_broadcast(&r->cv);
        pthread_mutex_unlock(&r->mu);
        if (got < cap)
            return NULL; /* end of file (or an error: the run ends there, air.c:236-237) */
    }
}

static double now_ms(void)
{
    struct timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec * 1e3 + ts.tv_nsec * 1e-6;
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
            s->registered = adsb_host_register(s->buf, buf_bytes) == 0;
            r->t_reg += now_ms() - t0;
        }
        pthread_mutex_lock(&r->mu);
        s->ready = 1;
        pthread_cond_broadcast(&r->cv);
        pthread_mutex_unlock(&r->mu);
        if (bytes < buf_bytes)
            return NULL;
    }
}

static void usage(void)
{
    printf("adsbdec_amd : MI355X offline ADS-B decoder (adsbdec -f compatible)\n\n");
    printf("usage : adsbdec_amd_cli [-a] [-m] [-b] [-p] [-t type] [-q type] [-w] [-E] [-s addr[:port] | -l addr[:port]] [-d gpu | -G gpus] -f filename [-f filename ...]\n");
    printf("        adsbdec_amd_cli [-a] [-m] [-b] [-p] [-E] [-d gpu | -G gpus] -B listfile\n");
    printf("        adsbdec_amd_cli [-q type] [-d gpu] -W out.pw -f filename\n");
    printf("        adsbdec_amd_cli [-p | -t type | -q type | -w] [-d gpu] -L -f filename\n");
    printf("        adsbdec_amd_cli [-d gpu] -L -I ms -f filename\n");
    printf("        adsbdec_amd_cli [-p | -t type | -q type | -w] [-d gpu] -L -U factor[,lead[,hang]] -f filename\n");
    printf("        adsbdec_amd_cli [-q type | -w] [-d gpu] -L -U factor[,lead[,hang]] -K out.brs -f filename\n");
    printf("        adsbdec_amd_cli [-p | -t type] [-d gpu] -L -U factor[,lead[,hang]] -P out.brs -f filename\n");
    printf("        adsbdec_amd_cli [-a] [-m] [-b] [-x] [-s addr[:port] | -l addr[:port]] [-d gpu] -k -f in.brs\n\n");
    printf("\t-a : decode DF18 too\n");
    printf("\t-m : output avrmlat format (ie : with 12Mhz timestamp)\n");
    printf("\t-b : output binary beast format\n");
    printf("\t-s addr[:port] : send ouput via TCP to addr:port (default port 30001)\n");
    printf("\t-l addr[:port] : listen to addr:port (default port 30002) and send ouput to the peer that connects\n");
    printf("\t-x : (extension) repair 1-bit CRC errors in DF17/18 frames\n");
    printf("\t-d k : (extension) use GPU k\n");
    printf("\t-p : (extension) the file holds Airspy packed 12-bit samples (8 samples in 12 bytes), unpacked on the GPU; not with -G\n");
    printf("\t-t type : (extension) sample type of the file as airspy_rx -t numbers it: 1 float32 real and 3 signed 16 bits real are\n");
    printf("\t     converted on the GPU, 4 and 5 are the uint16 code (the default); not 0 or 2 (IQ); 1 and 3 not with -p, -G or -B\n");
    printf("\t-q type : (extension) the file holds COMPLEX samples at 10 MS/s, as airspy_rx -t numbers them: 2 signed 16 bits IQ (airspy_rx's\n");
    printf("\t     default), 0 float32 IQ (quantised to the int16 grid on the GPU); not with -t, -p, -G or -B\n");
    printf("\t     -q 8 (not an airspy_rx number): signed 8 bits IQ, as hackrf_transfer -r writes (cs8 / sc8); not with -w or -W either\n");
    printf("\t-w : (extension) the file holds float32 POWER samples at 10 MS/s (little-endian), the demodulator's own input; every sample finite,\n");
    printf("\t     sign bit clear and below 2^29 (no negatives, -0.0, NaN, Inf; subnormals are fine); not with -t, -q, -p, -G or -B\n");
    printf("\t-W out.pw : (extension) export, do not decode: write the float32 power samples of the file (what -w reads) to out.pw; with -q the\n");
    printf("\t     file is IQ (any length; a real file: below 2^32 samples); not with -w, -t, -p, -G, -B, -s, -l or several -f\n");
    printf("\t-L : (extension) report the levels, do not decode: the file's power samples (what -W writes; with -w the file's own floats) as\n");
    printf("\t     counters (samples, negative, codes on the ADC's rails and above 4095), a histogram in bins of 1/8 octave (0.75 dB) and its\n");
    printf("\t     median, 99.9th percentile and peak in dB of raw power units; input as -p, -t, -q (8 too) or -w say; the whole file in one\n");
    printf("\t     call (a real file: below 2^32 samples, IQ and power: below 2^31); not with -G, -B, -W, -s, -l or several -f\n");
    printf("\t-I ms : (extension) with -L on a uint16 file: the levels over time.  A line per window of ms milliseconds (10 000 power samples\n");
    printf("\t     each, rounded down to a multiple of 28): its start in seconds, median, 99.9th percentile and peak, the three rail counters;\n");
    printf("\t     then -L's report of the whole.  The file is read in pieces of bounded size: a FIFO works; not with -t, -p, -q or -w\n");
    printf("\t-U factor[,lead[,hang]] : (extension) with -L: find the bursts.  Behind the report a line `bursts B threshold T lead L hang H` and a\n");
    printf("\t     line `first end hot peak` per burst, in power samples: the envelope (a float per 28 power samples) gated at factor x the\n");
    printf("\t     median, lead (default 2) and hang (default 1468: a piece must outlast the decoder's 40 980-sample horizon) runs kept; not with -I\n");
    printf("\t     (pieces decoded with -E, on a flush handle, have no horizon to outlast: hang 4 is enough for them)\n");
    printf("\t-K out.brs : (extension) with -L -U: keep only the bursts.  Behind the report and the burst lines the pieces the gate found are\n");
    printf("\t     gathered on the GPU out of the capture's own bytes (adsb_gather_device), copied back once and written to out.brs, a burst\n");
    printf("\t     archive (header, burst table, the pieces each from a multiple of 16 bytes on); stderr: `kept B bursts, X of Y bytes`; a\n");
    printf("\t     uint16, -q 2 | 0 | 8 or -w file; for an archive meant for -k, hang 4 is enough; not with -t, -p, -I, -G, -B or -W\n");
    printf("\t-P out.brs : (extension) with -L -U: keep only the bursts of a real capture, at 12 bits.  As -K, for a uint16 (default), -p or\n");
    printf("\t     -t 3 | 1 file: the pieces are packed on the GPU into Airspy packed 12-bit samples while they are gathered\n");
    printf("\t     (adsb_gather_pack12_*), 3 bytes per power sample where -K writes 4; archive kind 12, which -k decodes; stderr: `kept B\n");
    printf("\t     bursts, X of Y bytes`; a sample above 4095 inside a burst: status 255, no archive, use -K; not with -q, -w, -K, -I, -G,\n");
    printf("\t     -B, -W or -k\n");
    printf("\t-k : (extension) the file of -f is a burst archive: decode its pieces in one batch call, each to its last sample (as -E does),\n");
    printf("\t     and print the packets in order, positions counted in the original capture (a packet's 12 MHz timestamp is the\n");
    printf("\t     original's only up to the jumps of the frames accepted before its piece); the kind of the samples comes from the\n");
    printf("\t     header: not with -t, -p, -q, -w, -E, -G, -B, -L, -W or -K\n");
    printf("\t-E : (extension) decode to the file's last sample: the packets and the table of the file followed by 81 960 power samples of silence,\n");
    printf("\t     instead of leaving the last ~41 k power samples unscanned as adsbdec does (a file below 81 960 samples decodes nothing there);\n");
    printf("\t     every input kind of -f, and -B on one GPU; a real file below 2^32 samples; not with -G, -L or -W\n");
    printf("\t-G n | a,b,.. : (extension) shard the file over n GPUs / the GPUs listed; several -f: one capture per GPU,\n");
    printf("\t     packets of capture k written to <file k>.avr | .mlat | .beast\n");
    printf("\t-B listfile : (extension) a batch of captures, one path per line of listfile (any number; empty lines skipped):\n");
    printf("\t     decoded many per launch on the GPU of -d or the GPUs of -G, packets of capture k written to\n");
    printf("\t     <capture k>.avr | .mlat | .beast; -p allowed (all captures packed); not with -f, -s or -l\n");
    printf("\t-f : input from filename (raw 16 bits real: uint16 carrying the 12-bit ADC code centred on 2048;\n");
    printf("\t     bit-identical to adsbdec for codes 0..4095, see adsbdec_amd.h for the wider domain)\n");
    printf("\t     a file of any length: 2^32 samples (8 GiB) and more are decoded through the wraps of adsbdec's 32-bit\n");
    printf("\t     sample counter, as adsbdec itself does; one file sharded over several GPUs (-G) stays below 2^32 samples\n");
}

static sink out_sink; /* stdout unless -s / -l */

/* main.c:91-99: SIGINT / SIGTERM / SIGQUIT end the run in an orderly way -- the reference's handlerExit sets do_exit, the
 * writer loop ends, main prints the Try/Ok table and returns runOutput()'s 0 -- and SIGPIPE is ignored, so that a closed
 * stdout or peer shows up as a failed write, not as death by signal.  Here: the handler sets a flag (no SA_RESTART: a
 * blocking accept / connect / read returns), the push loop stops at the next buffer, what has been decoded is finished,
 * written and counted, the table is printed, exit status 0. */
static volatile int stop_requested;
static void on_stop_signal(int sig)
{
    (void)sig;
    stop_requested = 1;
}
static void install_signals(void)
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

/* Packets leave in batches of up to 64 KiB: one fwrite / send per batch. */
static int write_frames(sink *out, const adsb_frame *fr, long n, int outformat)
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

static int flush_frames(adsb_decoder *dec, int outformat)
{
    const adsb_frame *fr; /* the handle's own queue: formatted where it lies */
    const long n = adsb_take(dec, &fr);
    if (n < 0)
        return -1;
    return write_frames(&out_sink, fr, n, outformat);
}

static void print_stats(const adsb_stats *st) /* valid.c:84-100 */
{
    unsigned long long tot = st->ok[0] + st->ok[1] + st->ok[2];
    fprintf(stderr, "\t%10d\t%10d\t%10d\n", 11, 17, 18);
    fprintf(stderr, "Try :\t%10llu\t%10llu\t%10llu\n", (unsigned long long)st->try_[0], (unsigned long long)st->try_[1],
            (unsigned long long)st->try_[2]);
    fprintf(stderr, "Ok :\t%10llu\t%10llu\t%10llu\n", (unsigned long long)st->ok[0], (unsigned long long)st->ok[1],
            (unsigned long long)st->ok[2]);
    fprintf(stderr, "Total :\t%10llu\n", tot); /* tot_fi is uninitialised there */
}

static int write_frames_file(FILE *out, const adsb_frame *fr, long n, int outformat)
{
    char pkt[256];
    for (long i = 0; i < n; i++) {
        int len = adsb_format_frame(&fr[i], outformat, pkt);
        if (fwrite(pkt, 1, (size_t)len, out) != (size_t)len)
            return -1;
    }
    return 0;
}

#define MAX_GPUS 64
#define MAX_FILES 64

/* "-G 4" -> 0,1,2,3; "-G 0,2,2" -> as listed.  Returns the count, 0 on a malformed argument. */
static int parse_gpus(const char *arg, int *devs)
{
    int n = 0;
    if (!strchr(arg, ',')) {
        char *end;
        long k = strtol(arg, &end, 10);
        if (*end || k < 1 || k > MAX_GPUS)
            return 0;
        for (n = 0; n < k; n++)
            devs[n] = n;
        return n;
    }
    for (const char *p = arg; *p;) {
        char *end;
        long k = strtol(p, &end, 10);
        if (end == p || k < 0 || k > 1023 || n == MAX_GPUS)
            return 0;
        devs[n++] = (int)k;
        p = (*end == ',') ? end + 1 : end;
        if (*end && *end != ',')
            return 0;
    }
    return n;
}

/* Narrow the runtime's view to the devices in use, BEFORE its first call (it initialises every device it sees), and
 * renumber devs[] to the ordinals the runtime will then hand out.  A caller's own ROCR_VISIBLE_DEVICES is left alone. */
static void restrict_visible_devices(int *devs, int n)
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

/* -G: the library's multi-GPU driver.  One file: sharded over the devices, same bytes as the one-device run.  Several: one
 * capture per device, packets into <file>.<format>. */
static int run_multi(const adsb_config *cfg, int *devs, int ndev, char **files, int nfiles, int outformat, int timing)
{
    const double t_start = now_ms();
    adsb_multi *m = adsb_multi_create(cfg, ndev, devs);
    if (!m) {
        fprintf(stderr, "adsb_multi_create() failed: %s\n", adsb_multi_last_error(NULL));
        return 255;
    }
    const double t_init = now_ms();
    int rc = 0;
    if (nfiles == 1) {
        const adsb_frame *fr = NULL;
        const long n = adsb_multi_decode_file(m, files[0], &fr);
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
        if (adsb_multi_decode_streams_file(m, nfiles, (const char *const *)files) != 0) {
            fprintf(stderr, "adsb_multi_decode_streams_file() failed: %s\n", adsb_multi_last_error(m));
            rc = 255;
        }
        static const char *ext[3] = {"avr", "mlat", "beast"};
        for (int k = 0; k < nfiles && rc == 0; k++) {
            const adsb_frame *fr = NULL;
            const long n = adsb_multi_stream_frames(m, k, &fr);
            char path[4096];
            snprintf(path, sizeof path, "%s.%s", files[k], ext[outformat]);
            FILE *out = n >= 0 ? fopen(path, "wb") : NULL;
            if (!out || write_frames_file(out, fr, n, outformat) != 0 || fclose(out) != 0) {
                fprintf(stderr, "%s: cannot write\n", path);
                rc = 1;
                break;
            }
            adsb_stats st;
            fprintf(stderr, "== %s: %ld frames -> %s\n", files[k], n, path);
            if (adsb_multi_stream_stats(m, k, &st) == 0)
                print_stats(&st);
        }
        if (timing)
            fprintf(stderr, "timing: runtime init %.1f ms, decode %.1f ms, total %.1f ms\n", t_init - t_start, now_ms() - t_init,
                    now_ms() - t_start);
    }
    fflush(stderr);
    if (getenv("ADSB_CLI_CLEAN_EXIT"))
        exit(rc);
    _exit(rc); /* (no teardown: see the end of main) */
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

/* -B: every capture of the list through ONE start of the runtime and the library's batch calls; packets into <capture>.<format>. */
static int run_batch_list(const adsb_config *cfg, int *devs, int ndev, char **paths, size_t n_captures, int packed, int outformat,
                          int timing)
{
    static const char *ext[3] = {"avr", "mlat", "beast"};
    const double t_start = now_ms();
    adsb_multi *m = adsb_multi_create(cfg, ndev, devs);
    if (!m) {
        fprintf(stderr, "adsb_multi_create() failed: %s\n", adsb_multi_last_error(NULL));
        return 255;
    }
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
    for (size_t k = 0; k < n_captures && rc == 0; k++) {
        char path[4096];
        if ((size_t)snprintf(path, sizeof path, "%s.%s", paths[k], ext[outformat]) >= sizeof path) {
            fprintf(stderr, "%s: the name of its .%s file is longer than %zu bytes\n", paths[k], ext[outformat], sizeof path - 1);
            rc = 1;
            break;
        }
        const long n = (long)(first[k + 1] - first[k]);
        FILE *out = fopen(path, "wb");
        if (!out || write_frames_file(out, fr + first[k], n, outformat) != 0 || fclose(out) != 0) {
            fprintf(stderr, "%s: cannot write\n", path);
            rc = 1;
            break;
        }
        fprintf(stderr, "== %s: %ld frames -> %s\n", paths[k], n, path);
        print_stats(&st[k]);
    }
    if (timing) {
        adsb_multi_info inf;
        adsb_multi_get_info(m, &inf);
        fprintf(stderr, "timing: runtime init %.1f ms, decode of %zu captures %.1f ms (%d workers, slowest %.1f ms), writing %.1f ms, total %.1f ms\n",
                t_init - t_start, n_captures, t_decoded - t_init, inf.shards, inf.workers_ms, now_ms() - t_decoded, now_ms() - t_start);
    }
    fflush(stderr);
    if (getenv("ADSB_CLI_CLEAN_EXIT"))
        exit(rc);
    _exit(rc); /* (no teardown: see the end of main) */
}

/* read() until `want` bytes are in or the file ends */
static size_t read_full(int fd, void *buf, size_t want)
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

/* -B -E: the captures of the list, read whole into memory, through ONE batch call of a flush handle on one GPU (adsb_set_flush +
 * adsb_decode_batch_host / _host_packed); packets and tables go where run_batch_list puts them.  The multi-GPU driver has no flush. */
static int run_batch_list_flush(const adsb_config *cfg, char **paths, size_t n_captures, int packed, int outformat)
{
    static const char *ext[3] = {"avr", "mlat", "beast"};
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
    adsb_decoder *dec = adsb_create(cfg);
    if (!dec) {
        fprintf(stderr, "adsb_create() failed: %s\n", adsb_last_error(NULL));
        return 255;
    }
    const adsb_frame *fr = NULL;
    int rc = 0;
    if (adsb_set_flush(dec, 1) != 0 ||
        (packed ? adsb_decode_batch_host_packed(dec, n_captures, (const void *const *)buf, n, &fr, first, st)
                : adsb_decode_batch_host(dec, n_captures, (const uint16_t *const *)buf, n, &fr, first, st)) < 0) {
        fprintf(stderr, "the batch decode failed: %s\n", adsb_last_error(dec));
        rc = 255;
    }
    for (size_t k = 0; k < n_captures && rc == 0; k++) {
        char path[4096];
        if ((size_t)snprintf(path, sizeof path, "%s.%s", paths[k], ext[outformat]) >= sizeof path) {
            fprintf(stderr, "%s: the name of its .%s file is longer than %zu bytes\n", paths[k], ext[outformat], sizeof path - 1);
            rc = 1;
            break;
        }
        const long nf = (long)(first[k + 1] - first[k]);
        FILE *out = fopen(path, "wb");
        if (!out || write_frames_file(out, fr + first[k], nf, outformat) != 0 || fclose(out) != 0) {
            fprintf(stderr, "%s: cannot write\n", path);
            rc = 1;
            break;
        }
        fprintf(stderr, "== %s: %ld frames -> %s\n", paths[k], nf, path);
        print_stats(&st[k]);
    }
    fflush(stderr);
    if (getenv("ADSB_CLI_CLEAN_EXIT"))
        exit(rc);
    _exit(rc); /* (no teardown: see the end of main) */
}

/* -W: the file's power samples into `outpath`; nothing is decoded.  A piece of a uint16 file is EXPORT_PIECE power samples (a
 * multiple of 28: about 4 Mi samples) behind the last 16 samples of the piece before it; an IQ piece is EXPORT_PIECE complex samples. */
#define EXPORT_PIECE ((uint64_t)28 * 74898)
#define EXPORT_OVERLAP 16
static int run_export(const char *filename, const char *outpath, int device, int iq, int qtype)
{
    const int fd = open(filename, O_RDONLY);
    if (fd < 0) {
        fprintf(stderr, "%s: cannot read: %s\n", filename, strerror(errno));
        return 255;
    }
    adsb_config cfg;
    adsb_config_default(&cfg);
    cfg.device = device;
    adsb_decoder *dec = adsb_create(&cfg);
    if (!dec) {
        fprintf(stderr, "adsb_create() failed: %s\n", adsb_last_error(NULL));
        return 255;
    }
    FILE *out = fopen(outpath, "wb"); /* (behind adsb_create: no empty file is left where no GPU is) */
    if (!out) {
        fprintf(stderr, "%s: cannot write: %s\n", outpath, strerror(errno));
        return 255;
    }
    int rc = 0;
    float *pw = (float *)malloc(EXPORT_PIECE * sizeof(float));
    if (!iq) {
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
    fflush(stderr);
    if (getenv("ADSB_CLI_CLEAN_EXIT"))
        exit(rc);
    _exit(rc); /* (no teardown: see the end of main) */
}

/* -L: the level report of the file's power samples on stdout; nothing is decoded.  The whole file is ONE capture in ONE call (the
 * report of a real capture needs every pair's six predecessors, and only the uint16 flavour has a window call: -I, run_level_windows below): kind 0 uint16 (adsb_level_host,
 * through the handle's buffers), 1 -t 1 | 3, 2 -p, 3 -q, 4 -w (a device buffer of the program's own). */
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

/* the report as -L prints it: the counters, a line per non-empty bin, the summary */
static void print_level_report(const adsb_level_report *rep)
{
    printf("samples %llu negative %llu rail_lo %llu rail_hi %llu over %llu\n", (unsigned long long)rep->samples, (unsigned long long)rep->negative,
           (unsigned long long)rep->rail_lo, (unsigned long long)rep->rail_hi, (unsigned long long)rep->over);
    unsigned peak = 0;
    uint64_t counted = 0;
    for (unsigned k = 0; k < 2048; k++) {
        if (!rep->hist[k])
            continue;
        union { uint32_t u; float f; } edge;
        edge.u = k << 20;
        if (k < 2040)
            printf("bin %u %.9g %llu\n", k, (double)edge.f, (unsigned long long)rep->hist[k]);
        else
            printf("bin %u %s %llu\n", k, k == 2040 ? "inf" : "nan", (unsigned long long)rep->hist[k]);
        peak = k;
        counted += rep->hist[k];
    }
    if (counted) { /* (dB of raw power units, not dBFS: nobody has measured the front end's gain) */
        print_db("median", bin_of_quantile(rep, 0.5), " ");
        print_db("p99.9", bin_of_quantile(rep, 0.999), " ");
        print_db("peak", peak, "\n");
    } else {
        printf("median none p99.9 none peak none\n");
    }
}

struct burst_opts { /* -U: factor 0 = no gate */
    double factor;
    uint32_t lead, hang;
};

/* -L -U: the gate behind the report.  env: the device array of ceil(m / 28) floats the level call wrote.  keep (-K; else NULL): the
 * table, its length and the threshold stay with the caller, who frees the table. */
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

/* -K: the pieces the table names, out of the capture the level call has read in HBM -- ONE adsb_gather_device call, ONE copy back,
 * the archive (burst_archive.h).  s: bytes per power sample of the capture's kind. */
static int keep_bursts(adsb_decoder *dec, const char *path, const void *d_in, size_t used, uint32_t kind, uint64_t n_units, uint64_t m,
                       const struct kept_bursts *k, const struct burst_opts *u)
{
    brs_archive a;
    memset(&a, 0, sizeof a);
    a.kind = kind, a.sample_bytes = brs_sample_bytes(kind);
    a.n_units = n_units, a.m = m;
    a.threshold = k->threshold, a.lead = u->lead, a.hang = u->hang;
    a.n_bursts = k->n, a.bursts = k->tab;
    char why[512];
    uint64_t total = 0;
    if (adsb_gather_layout(m, (int)a.sample_bytes, k->tab, k->n, NULL, &total) != 0) {
        fprintf(stderr, "adsb_gather_layout() failed: %s\n", adsb_last_error(NULL));
        return 255;
    }
    void *d_out = NULL;
    unsigned char *out = (unsigned char *)malloc(total ? (size_t)total : 1);
    int rc = 255; /* (one way out: what was allocated here is released on it) */
    long got;
    if (!out || (total && hipMalloc(&d_out, (size_t)total) != hipSuccess)) {
        d_out = NULL;
        fprintf(stderr, "cannot allocate the %llu bytes of the %zu bursts, on the host and on the device\n", (unsigned long long)total, k->n);
    } else if ((got = adsb_gather_device(dec, d_in, used, (int)a.sample_bytes, m, k->tab, k->n, d_out, (size_t)total, NULL)) < 0 ||
               (uint64_t)got != total) {
        fprintf(stderr, "adsb_gather_device() failed: %s\n", got < 0 ? adsb_last_error(dec) : "another total than the layout's");
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

/* -P: the same out of the capture's uint16 twin, packed to 12 bits while it is gathered -- ONE adsb_gather_pack12_* call of the file's
 * flavour (kind 0: uint16; 1: -t fmt; 2: -p), ONE copy back, the archive of kind 12.  A piece's own sample above 4095: no archive. */
static int keep_bursts_pack12(adsb_decoder *dec, const char *path, int kind, int fmt, const void *d_in, size_t n, uint64_t m,
                              const struct kept_bursts *k, const struct burst_opts *u)
{
    brs_archive a;
    memset(&a, 0, sizeof a);
    a.kind = BRS_KIND_PACKED12_REAL, a.sample_bytes = brs_sample_bytes(BRS_KIND_PACKED12_REAL);
    a.n_units = n, a.m = m;
    a.threshold = k->threshold, a.lead = u->lead, a.hang = u->hang;
    a.n_bursts = k->n, a.bursts = k->tab;
    char why[512];
    uint64_t total = 0, over = 0;
    if (adsb_gather_pack12_layout(m, k->tab, k->n, NULL, &total) != 0) {
        fprintf(stderr, "adsb_gather_pack12_layout() failed: %s\n", adsb_last_error(NULL));
        return 255;
    }
    void *d_out = NULL;
    unsigned char *out = (unsigned char *)malloc(total ? (size_t)total : 1);
    int rc = 255; /* (one way out: what was allocated here is released on it) */
    long got = -1;
    if (!out || (total && hipMalloc(&d_out, (size_t)total) != hipSuccess)) {
        d_out = NULL;
        fprintf(stderr, "cannot allocate the %llu bytes of the %zu bursts, on the host and on the device\n", (unsigned long long)total, k->n);
    } else if ((got = kind == 1   ? adsb_gather_pack12_device_as(dec, fmt, d_in, n, k->tab, k->n, d_out, (size_t)total, NULL, &over)
                      : kind == 2 ? adsb_gather_pack12_device_packed(dec, d_in, n, k->tab, k->n, d_out, (size_t)total, NULL, &over)
                                  : adsb_gather_pack12_device(dec, d_in, n, k->tab, k->n, d_out, (size_t)total, NULL, &over)) < 0 ||
               (uint64_t)got != total) {
        fprintf(stderr, "adsb_gather_pack12_device%s() failed: %s\n", kind == 1 ? "_as" : kind == 2 ? "_packed" : "",
                got < 0 ? adsb_last_error(dec) : "another total than the layout's");
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

static int run_level(const char *filename, int device, int kind, int fmt, const struct burst_opts *u, const char *archive_out, int pack12)
{
    const int fd = open(filename, O_RDONLY);
    struct stat sb;
    if (fd < 0 || fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) {
        fprintf(stderr, "%s: cannot read as a regular file: %s\n", filename, fd < 0 ? strerror(errno) : "-L takes the whole file in one call");
        return 255;
    }
    adsb_config cfg;
    adsb_config_default(&cfg);
    cfg.device = device;
    adsb_decoder *dec = adsb_create(&cfg);
    if (!dec) {
        fprintf(stderr, "adsb_create() failed: %s\n", adsb_last_error(NULL));
        return 255;
    }
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
    const int gate = u->factor > 0;
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
        struct kept_bursts kept = {NULL, 0, 0};
        int rc = print_bursts(dec, rep, d_env, (uint64_t)got, u, archive_out ? &kept : NULL);
        if (rc == 0 && archive_out && pack12) { /* (main has refused -P with -q and -w: kind is 0, 1 or 2 here) */
            fflush(stdout);
            rc = keep_bursts_pack12(dec, archive_out, kind, fmt, d_in, n, (uint64_t)got, &kept, u);
        } else if (rc == 0 && archive_out) { /* (main has refused -K with -t and -p: kind is 0, 3 or 4 here) */
            fflush(stdout);
            rc = keep_bursts(dec, archive_out, d_in, used, kind == 0 ? BRS_KIND_UINT16_REAL : kind == 4 ? BRS_KIND_FLOAT32_POWER : (uint32_t)fmt,
                             (uint64_t)n, (uint64_t)got, &kept, u);
        }
        free(kept.tab);
        if (rc) {
            fflush(stdout);
            return rc;
        }
    }
    fflush(stdout);
    fflush(stderr);
    if (getenv("ADSB_CLI_CLEAN_EXIT"))
        exit(0);
    _exit(0); /* (no teardown: see the end of main) */
}

/* -L -I ms: the levels over time.  The file -- a FIFO will do -- is read in pieces of LEVEL_PIECE power samples at most, each behind the
 * last 16 samples of the piece before it, so that every power sample has its six older pairs; a piece is ONE adsb_level_windows_host
 * call over windows of `ms` milliseconds (10 000 power samples each, rounded down to a multiple of 28).  A line per window, then -L's
 * own report of their sum (adsb_level_add). */
#define LEVEL_PIECE ((uint64_t)28 * 299593) /* about 16 Mi samples */
#define LEVEL_PIECE_WINDOWS 1024            /* one launch (adsbdec_amd.h) */
#define LEVEL_OVERLAP 16
static int run_level_windows(const char *filename, int device, double ms)
{
    const double per_ms = 10000.0; /* power samples: 20 MS/s real, a power sample per pair */
    const uint64_t win = ms * per_ms >= (double)LEVEL_PIECE ? LEVEL_PIECE : (uint64_t)(ms * per_ms) / 28 * 28;
    if (win == 0) {
        fprintf(stderr, "-I %g: a window holds at least 28 power samples (0.0028 ms)\n", ms);
        return 1;
    }
    if (ms * per_ms > (double)LEVEL_PIECE)
        fprintf(stderr, "-I %g: windows of %llu power samples (%.4f ms), the most this program reads at once\n", ms, (unsigned long long)win,
                (double)win / per_ms);
    const int fd = open(filename, O_RDONLY);
    if (fd < 0) {
        fprintf(stderr, "%s: cannot read: %s\n", filename, strerror(errno));
        return 255;
    }
    adsb_config cfg;
    adsb_config_default(&cfg);
    cfg.device = device;
    adsb_decoder *dec = adsb_create(&cfg);
    if (!dec) {
        fprintf(stderr, "adsb_create() failed: %s\n", adsb_last_error(NULL));
        return 255;
    }
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
            unsigned peak = 0, any = 0;
            for (unsigned b = 0; b < 2048; b++)
                if (r->hist[b])
                    peak = b, any = 1;
            printf("t %.6f s ", (double)edges[i] / (per_ms * 1000.0));
            if (any) {
                print_db("median", bin_of_quantile(r, 0.5), " ");
                print_db("p99.9", bin_of_quantile(r, 0.999), " ");
                print_db("peak", peak, " ");
            } else {
                printf("median none p99.9 none peak none ");
            }
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
    fflush(stderr);
    if (getenv("ADSB_CLI_CLEAN_EXIT"))
        exit(0);
    _exit(0); /* (no teardown: see the end of main) */
}

/* -k: decode a burst archive.  The pieces go through ONE adsb_decode_batch_host* call of the archive's kind on a flush handle (a piece
 * is far below the end-of-file horizon), pointers payload + offsets[i]; piece i's packets are its silent twin's, written in order with
 * g + 28 begin_i -- exact -- and ts + 28 begin_i: in the original stream ts lags g by what accepted frames have jumped
 * (demod.c:99,128,134), so this is the original's ts only up to those jumps.  The table is the sum of the pieces' tables. */
static int run_archive(const char *filename, const adsb_config *cfg, int outformat)
{
    brs_archive a;
    char why[512];
    if (brs_read(filename, &a, why, sizeof why) != 0) {
        fprintf(stderr, "%s: %s\n", filename, why);
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
    {
        const int prc = sink_wait_peer(&out_sink);
        if (prc == 2) { /* told to end before a peer came */
            adsb_stats z;
            memset(&z, 0, sizeof z);
            print_stats(&z);
            fflush(stderr);
            _exit(0);
        }
        if (prc != 0)
            return 255;
    }
    adsb_decoder *dec = adsb_create(cfg);
    if (!dec) {
        fprintf(stderr, "adsb_create() failed: %s\n", adsb_last_error(NULL));
        return 255;
    }
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
    if (write_frames(&out_sink, mine, total, outformat) != 0)
        rc = 1;
    if (sink_close(&out_sink) != 0 && rc == 0)
        rc = 1;
    print_stats(&sum);
    fflush(stderr);
    if (getenv("ADSB_CLI_CLEAN_EXIT"))
        exit(rc);
    _exit(rc); /* (no teardown: see the end of main) */
}

int main(int argc, char **argv)
{
    const char *filename = NULL, *listfile = NULL, *export_path = NULL;
    char *files[MAX_FILES];
    int nfiles = 0, devs[MAX_GPUS], ndev = 0, device = -1;
    int outformat = 0, df18 = 0, fix1 = 0, packed = 0, power = 0, level = 0, flush = 0, c;
    const char *burst_arg = NULL; /* -U: -L's gate, factor[,lead[,hang]] */
    struct burst_opts burst = {0, 2, 1468};
    const char *archive_out = NULL; /* -K: keep only the bursts of -L -U, as a burst archive */
    const char *pack_out = NULL;    /* -P: ... of a real capture, packed to 12 bits (archive kind 12) */
    int archive_in = 0;             /* -k: the file of -f is a burst archive */
    const char *interval_arg = NULL; /* -I: -L's windows, in milliseconds */
    double interval_ms = 0;
    long stype = 5; /* -t: ADSB_FMT_RAW */
    const char *stype_arg = NULL;
    long qtype = -1; /* -q: ADSB_FMT_INT16_IQ / ADSB_FMT_FLOAT32_IQ / ADSB_FMT_INT8_IQ */
    const char *qtype_arg = NULL;
    int outmode = SINK_STDOUT;
    const char *rawaddr = NULL;

    while ((c = getopt(argc, argv, "f:g:ambxpwd:G:s:l:B:t:q:W:LI:U:EK:kP:")) != EOF) {
        switch (c) {
        case 'f':
            filename = optarg;
            if (nfiles == MAX_FILES) { /* (more captures than this program keeps track of: say so, do not drop them) */
                usage();
                return 1;
            }
            files[nfiles++] = optarg;
            break;
        case 'B':
            listfile = optarg;
            break;
        case 'd': {
            char *end;
            long k = strtol(optarg, &end, 10);
            if (*end || k < 0 || k > 1023) {
                usage();
                return 1;
            }
            device = (int)k;
            break;
        }
        case 'G':
            ndev = parse_gpus(optarg, devs);
            if (ndev == 0) {
                usage();
                return 1;
            }
            break;
        case 's':
            rawaddr = optarg;
            outmode = SINK_CONNECT;
            break;
        case 'l':
            rawaddr = optarg;
            outmode = SINK_LISTEN;
            break;
        case 'g':
            break;
        case 'a':
            df18 = 1;
            break;
        case 'm':
            outformat = 1;
            break;
        case 'b':
            outformat = 2;
            break;
        case 'x':
            fix1 = 1;
            break;
        case 'p':
            packed = 1;
            break;
        case 'w':
            power = 1;
            break;
        case 'W':
            export_path = optarg;
            break;
        case 'L':
            level = 1;
            break;
        case 'E':
            flush = 1;
            break;
        case 'K':
            archive_out = optarg;
            break;
        case 'k':
            archive_in = 1;
            break;
        case 'P':
            pack_out = optarg;
            break;
        case 'I': {
            char *end;
            interval_ms = strtod(optarg, &end);
            if (*end || end == optarg || !(interval_ms > 0) || interval_ms > 1e12)
                interval_ms = 0;
            interval_arg = optarg;
            break;
        }
        case 'U': { /* factor[,lead[,hang]]: a finite factor above 0, whole numbers up to 2^30; anything else leaves factor 0 */
            char *end;
            burst_arg = optarg;
            burst.factor = strtod(optarg, &end);
            int ok = end != optarg && burst.factor > 0 && burst.factor <= 1.7976931348623157e308;
            uint32_t *field[2] = {&burst.lead, &burst.hang};
            for (int i = 0; ok && i < 2 && *end == ','; i++) {
                const char *at = end + 1;
                const unsigned long long v = strtoull(at, &end, 10);
                ok = end != at && *at >= '0' && *at <= '9' && v <= (1ull << 30);
                *field[i] = (uint32_t)v;
            }
            if (!ok || *end)
                burst.factor = 0;
            break;
        }
        case 't': {
            char *end;
            stype = strtol(optarg, &end, 10);
            if (*end || end == optarg)
                stype = -1;
            stype_arg = optarg;
            break;
        }
        case 'q': {
            char *end;
            qtype = strtol(optarg, &end, 10);
            if (*end || end == optarg)
                qtype = -1;
            qtype_arg = optarg;
            break;
        }
        default:
            usage();
            return 1;
        }
    }
    if (pack_out && (!level || !burst_arg || qtype_arg || power || archive_out || interval_arg || ndev || listfile || export_path || archive_in)) {
        /* -P keeps the pieces -L -U finds of a REAL capture, packed to 12 bits: refused before any GPU call */
        if (!level || !burst_arg)
            fprintf(stderr, "-P is not supported without -L -U: it keeps the bursts that the gate behind the level report finds\n");
        else
            fprintf(stderr, "-P is not supported with %s: %s\n",
                    qtype_arg ? "-q" : power ? "-w" : archive_out ? "-K" : interval_arg ? "-I" : ndev ? "-G" : listfile ? "-B" : export_path ? "-W" : "-k",
                    qtype_arg || power  ? "12-bit codes are what a REAL capture carries (a uint16 file, -p or -t 3 | 1); -K keeps IQ and power samples as they are"
                    : archive_out       ? "a run writes one archive: the capture's own bytes (-K) or its 12-bit codes (-P)"
                    : interval_arg      ? "the windows are pieces of a stream, and joining bursts across pieces is the caller's: one file, one call"
                    : ndev || listfile  ? "the gather runs on one GPU (-d), one file at a time: no batch and no multi-GPU form"
                    : export_path       ? "a run writes the power samples or keeps the capture's bursts, not both"
                                        : "-k reads an archive, -P writes one");
        return 1;
    }
    if (archive_in && (stype_arg || packed || qtype_arg || power || flush || ndev || listfile || level || export_path || archive_out || nfiles > 1)) {
        /* -k decodes a burst archive, whose header says what it holds: refused before any GPU call */
        fprintf(stderr, "-k is not supported with %s: %s\n",
                stype_arg ? "-t" : packed ? "-p" : qtype_arg ? "-q" : power ? "-w" : flush ? "-E" : ndev ? "-G" : listfile ? "-B" : level ? "-L"
                : export_path ? "-W" : archive_out ? "-K" : "several -f",
                stype_arg || packed || qtype_arg || power ? "the kind of the samples comes from the archive's header"
                : flush                                    ? "an archive is always decoded to the last sample of every piece"
                : ndev || listfile                         ? "an archive is decoded on one GPU (-d) by one batch call: no multi-GPU and no list form"
                : level || export_path || archive_out      ? "the pieces of an archive are decoded, not measured, exported or gathered again"
                                                           : "one archive at a time");
        return 1;
    }
    if (archive_out && (!level || !burst_arg || stype_arg || packed || interval_arg || ndev || listfile || export_path)) {
        /* -K keeps the pieces -L -U finds, out of the capture's own bytes: refused before any GPU call */
        if (!level || !burst_arg)
            fprintf(stderr, "-K is not supported without -L -U: it keeps the bursts that the gate behind the level report finds\n");
        else
            fprintf(stderr, "-K is not supported with %s: %s\n",
                    stype_arg ? "-t" : packed ? "-p" : interval_arg ? "-I" : ndev ? "-G" : listfile ? "-B" : "-W",
                    stype_arg || packed ? "the pieces of a converted or packed capture are not in the capture's own bytes (adsb_gather_device reads those)"
                    : interval_arg      ? "the windows are pieces of a stream, and joining bursts across pieces is the caller's: one file, one call"
                    : ndev || listfile  ? "the gather runs on one GPU (-d), one file at a time: no batch and no multi-GPU form"
                                        : "a run writes the power samples or keeps the capture's bursts, not both");
        return 1;
    }
    if (flush && (ndev || level || export_path)) {
        /* -E ends a decode on one GPU past the horizon: refused before any GPU call */
        fprintf(stderr, "-E is not supported with %s: %s\n", ndev ? "-G" : level ? "-L" : "-W",
                ndev ? "the multi-GPU driver stitches its shards at the reference's end-of-file horizon; -E decodes on one GPU (-d)"
                     : "it ends a DECODE at the file's last sample, and this run decodes nothing");
        return 1;
    }
    if (level && (ndev || listfile || export_path || outmode != SINK_STDOUT || nfiles > 1)) {
        /* -L reports the levels of one file in one call and decodes nothing: refused before any GPU call */
        fprintf(stderr, "-L is not supported with %s: %s\n",
                ndev ? "-G" : listfile ? "-B" : export_path ? "-W" : outmode == SINK_CONNECT ? "-s" : outmode == SINK_LISTEN ? "-l" : "several -f",
                ndev || listfile         ? "the level report runs on one GPU (-d), one file at a time: no batch and no multi-GPU form"
                : export_path            ? "a run writes the power samples or reports their levels, not both"
                : outmode != SINK_STDOUT ? "the report is text on stdout, not packets for a peer"
                                         : "the report is of one file");
        return 1;
    }
    if (interval_arg && (!level || stype_arg || packed || qtype_arg || power || interval_ms == 0)) {
        /* -I cuts -L's report of a uint16 file into windows: refused before any GPU call */
        if (!level)
            fprintf(stderr, "-I is not supported without -L: it is the length of the level report's windows\n");
        else if (stype_arg || packed || qtype_arg || power)
            fprintf(stderr, "-I is not supported with %s: the windows are of a uint16 file (adsb_level_windows); a slice of an IQ or power file is "
                            "already exact on its own\n", stype_arg ? "-t" : packed ? "-p" : qtype_arg ? "-q" : "-w");
        else
            fprintf(stderr, "-I %s: the windows' length in milliseconds, a number above 0\n", interval_arg);
        return 1;
    }
    if (burst_arg && (!level || interval_arg || !(burst.factor > 0))) {
        /* -U gates the envelope of -L's one call: refused before any GPU call (-L's own refusals, -G, -B and -W among them, stay in front) */
        if (!level)
            fprintf(stderr, "-U is not supported without -L: it gates the envelope the level report's call writes%s\n",
                    ndev ? " (and not with -G)" : listfile ? " (and not with -B)" : export_path ? " (and not with -W)" : "");
        else if (interval_arg)
            fprintf(stderr, "-U is not supported with -I: the windows share one envelope piece by piece, and joining bursts across pieces is the caller's\n");
        else
            fprintf(stderr, "-U %s: factor[,lead[,hang]] -- a finite factor above 0, lead and hang whole numbers of runs up to 2^30\n", burst_arg);
        return 1;
    }
    if (qtype_arg && qtype == ADSB_FMT_INT8_IQ && (stype_arg || packed || ndev || listfile || power || export_path)) {
        /* int8 IQ is decoded from one file on one GPU and nothing else: refused before any GPU call */
        fprintf(stderr, "-q 8 is not supported with %s: %s\n", stype_arg ? "-t" : packed ? "-p" : ndev ? "-G" : listfile ? "-B" : power ? "-w" : "-W",
                stype_arg ? "a file holds real samples (-t) or IQ samples (-q), not both"
                : packed  ? "a file is packed 12-bit real or IQ, not both"
                : power   ? "a file holds IQ samples (-q) or power samples (-w), not both"
                : export_path ? "the export reads uint16 codes, int16 IQ (-q 2) or float32 IQ (-q 0); an int8 sample's power is 256 (I^2 + Q^2)"
                          : "the multi-GPU driver reads uint16 and packed files only");
        return 1;
    }
    if (export_path && (power || stype_arg || packed || ndev || listfile || outmode != SINK_STDOUT || nfiles > 1)) {
        /* -W writes power samples and decodes nothing: refused before any GPU call */
        fprintf(stderr, "-W is not supported with %s: %s\n",
                power ? "-w" : stype_arg ? "-t" : packed ? "-p" : ndev ? "-G" : listfile ? "-B" : outmode == SINK_CONNECT ? "-s" : outmode == SINK_LISTEN ? "-l" : "several -f",
                power                    ? "a file of power samples is already what -W writes"
                : stype_arg              ? "the export reads uint16 codes (or IQ samples with -q); python -m adsbdec_amd.sample_formats converts other real types"
                : packed                 ? "the export reads uint16 codes (or IQ samples with -q); python -m adsbdec_amd.packed12 unpacks"
                : ndev || listfile       ? "the export runs on one GPU (-d), one file at a time"
                : outmode != SINK_STDOUT ? "power samples go to the file named, not to a peer"
                                         : "the export writes one file");
        return 1;
    }
    const int converted = stype == ADSB_FMT_FLOAT32_REAL || stype == ADSB_FMT_INT16_REAL;
    if (stype_arg && !converted && stype != ADSB_FMT_UINT16_REAL && stype != ADSB_FMT_RAW) {
        if (stype == 0 || stype == 2)
            fprintf(stderr, "-t %ld (%s) is not a real sample type: libairspy has already mixed, filtered and decimated an IQ stream, so it has no "
                            "raw twin to be decoded as; -t takes 1 (float32 real), 3 (int16 real), 4 or 5 (uint16)\n",
                    stype, stype == 0 ? "FLOAT32_IQ" : "INT16_IQ");
        else
            fprintf(stderr, "-t %s: unknown sample type; -t takes 1 (float32 real), 3 (int16 real), 4 or 5 (uint16)\n", stype_arg);
        return 1;
    }
    if (converted && (packed || ndev || listfile)) {
        fprintf(stderr, "-t %ld is not supported with %s: %s\n", stype, packed ? "-p" : ndev ? "-G" : "-B",
                packed ? "a file is packed 12-bit or of that type, not both" : "the multi-GPU driver reads uint16 and packed files only");
        return 1;
    }
    if (qtype_arg && qtype != ADSB_FMT_INT16_IQ && qtype != ADSB_FMT_FLOAT32_IQ && qtype != ADSB_FMT_INT8_IQ) {
        fprintf(stderr, "-q %s: not an IQ sample type; -q takes 2 (int16 IQ), 0 (float32 IQ) or 8 (int8 IQ), real samples go with -t\n", qtype_arg);
        return 1;
    }
    if (qtype_arg && (stype_arg || packed || ndev || listfile)) {
        fprintf(stderr, "-q %ld is not supported with %s: %s\n", qtype, stype_arg ? "-t" : packed ? "-p" : ndev ? "-G" : "-B",
                stype_arg ? "a file holds real samples (-t) or IQ samples (-q), not both"
                : packed  ? "a file is packed 12-bit real or IQ, not both"
                          : "the multi-GPU driver reads uint16 and packed files only");
        return 1;
    }
    if (power && (stype_arg || qtype_arg || packed || ndev || listfile)) {
        fprintf(stderr, "-w is not supported with %s: %s\n", stype_arg ? "-t" : qtype_arg ? "-q" : packed ? "-p" : ndev ? "-G" : "-B",
                stype_arg    ? "a file holds real samples (-t) or power samples (-w), not both"
                : qtype_arg  ? "a file holds IQ samples (-q) or power samples (-w), not both"
                : packed     ? "a file is packed 12-bit real or float32 power, not both"
                             : "the multi-GPU driver reads uint16 and packed files only");
        return 1;
    }
    const int iq = qtype_arg != NULL;
    if (listfile) { /* a batch: its own inputs and outputs -- no -f, no peer; -d and -G exclude each other here too */
        if (filename || outmode != SINK_STDOUT || (ndev && device >= 0)) {
            usage();
            return 1;
        }
        size_t n_captures = 0;
        char **paths = read_list(listfile, &n_captures);
        if (!paths)
            return 255;
        install_signals();
        if (ndev == 0) {
            devs[0] = device >= 0 ? device : 0;
            ndev = 1;
        }
        restrict_visible_devices(devs, ndev);
        adsb_config bcfg;
        adsb_config_default(&bcfg);
        bcfg.df18 = df18;
        bcfg.fix_1bit = fix1;
        bcfg.collect_stats = 1; /* the reference always prints Try/Ok */
        if (flush) {
            bcfg.device = devs[0]; /* (restrict_visible_devices has renumbered it where it narrowed the runtime's view) */
            return run_batch_list_flush(&bcfg, paths, n_captures, packed, outformat);
        }
        return run_batch_list(&bcfg, devs, ndev, paths, n_captures, packed, outformat, getenv("ADSB_CLI_TIMING") != NULL);
    }
    /* several captures need -G and go to files; -d and -G exclude each other */
    if (!filename || (nfiles > 1 && (ndev == 0 || outmode != SINK_STDOUT)) || (ndev && device >= 0)) {
        usage();
        return 1;
    }
    if (level) {
        if (device >= 0) {
            restrict_visible_devices(&device, 1);
        } else if (!getenv("ROCR_VISIBLE_DEVICES") && !getenv("HIP_VISIBLE_DEVICES") && !getenv("ADSB_CLI_ALL_DEVICES")) {
            int first = 0;
            restrict_visible_devices(&first, 1);
        }
        if (interval_arg)
            return run_level_windows(filename, device, interval_ms);
        return run_level(filename, device, converted ? 1 : packed ? 2 : iq ? 3 : power ? 4 : 0, iq ? (int)qtype : (int)stype, &burst, pack_out ? pack_out : archive_out,
                         pack_out != NULL);
    }
    if (export_path) {
        install_signals();
        if (device >= 0) {
            restrict_visible_devices(&device, 1);
        } else if (!getenv("ROCR_VISIBLE_DEVICES") && !getenv("HIP_VISIBLE_DEVICES") && !getenv("ADSB_CLI_ALL_DEVICES")) {
            int first = 0;
            restrict_visible_devices(&first, 1);
        }
        return run_export(filename, export_path, device, iq, (int)qtype);
    }
    if (archive_in) {
        install_signals();
        sink_init(&out_sink, outmode, rawaddr);
        out_sink.stop = &stop_requested;
        if (getenv("ADSB_CLI_RETRY_S"))
            out_sink.retry_s = (unsigned)atoi(getenv("ADSB_CLI_RETRY_S"));
        if (device >= 0) {
            restrict_visible_devices(&device, 1);
        } else if (!getenv("ROCR_VISIBLE_DEVICES") && !getenv("HIP_VISIBLE_DEVICES") && !getenv("ADSB_CLI_ALL_DEVICES")) {
            int first = 0;
            restrict_visible_devices(&first, 1);
        }
        adsb_config kcfg;
        adsb_config_default(&kcfg);
        kcfg.df18 = df18;
        kcfg.fix_1bit = fix1;
        kcfg.collect_stats = 1; /* the reference always prints Try/Ok */
        kcfg.device = device;
        return run_archive(filename, &kcfg, outformat);
    }
    if (packed && ndev) {
        fprintf(stderr, "-p (packed 12-bit input) is not supported with -G: the multi-GPU driver reads uint16 files only\n");
        return 1;
    }
    if (packed)
        buf_bytes = (size_t)BUF_SAMPLES / 8 * 12;
    const size_t elem = power ? sizeof(float) : iq ? adsb_iq_bytes((int)qtype, 1) : converted ? adsb_format_bytes((int)stype, 1) : 2; /* (host arithmetic: no GPU call) */
    if (converted)
        buf_bytes = adsb_format_bytes((int)stype, BUF_SAMPLES);
    if (iq)
        buf_bytes = adsb_iq_bytes((int)qtype, BUF_SAMPLES / 2);
    if (power)
        buf_bytes = sizeof(float) * (BUF_SAMPLES / 2);
    install_signals();
    sink_init(&out_sink, outmode, rawaddr);
    out_sink.stop = &stop_requested;
    if (getenv("ADSB_CLI_RETRY_S")) /* (a test's knob: the reference waits 3 s between attempts, output.c:282) */
        out_sink.retry_s = (unsigned)atoi(getenv("ADSB_CLI_RETRY_S"));

    const int timing = getenv("ADSB_CLI_TIMING") ? (atoi(getenv("ADSB_CLI_TIMING")) > 1 ? 2 : 1) : 0;
    if (ndev) {
        adsb_config mcfg;
        adsb_config_default(&mcfg);
        mcfg.df18 = df18;
        mcfg.fix_1bit = fix1;
        mcfg.collect_stats = 1; /* the reference always prints Try/Ok */
        /* The driver cuts FILES into slices (every device preads its own): what the reference accepts beyond that goes the
         * way the one-device run goes it -- a single -f that is a pipe, a FIFO or a device node is streamed through one
         * device (the first one listed), a single -f that cannot be opened ends the run silently with an empty table
         * (air.c:225-228), same bytes on stdout and stderr either way. */
        struct stat sb;
        const int one_ok = nfiles > 1 || (stat(files[0], &sb) == 0 && S_ISREG(sb.st_mode) && access(files[0], R_OK) == 0);
        if (one_ok) {
            restrict_visible_devices(devs, ndev);
            const int prc = sink_wait_peer(&out_sink);
            if (prc == 2) { /* told to end before a peer came: nothing decoded, the table (all zero) and status 0 (main.c:101-105) */
                adsb_stats z;
                memset(&z, 0, sizeof z);
                print_stats(&z);
                return 0;
            }
            if (prc != 0)
                return 255; /* unusable address: runOutput() == -1 (output.c:278-279) */
            return run_multi(&mcfg, devs, ndev, files, nfiles, outformat, timing);
        }
        device = devs[0];
        ndev = 0;
    }
    if (device >= 0) {
        restrict_visible_devices(&device, 1);
    } else if (!getenv("ROCR_VISIBLE_DEVICES") && !getenv("HIP_VISIBLE_DEVICES") && !getenv("ADSB_CLI_ALL_DEVICES")) {
        int first = 0;
        restrict_visible_devices(&first, 1); /* one device is all this run uses: do not start the others */
    }
    const int use_register = !(getenv("ADSB_CLI_REGISTER") && atoi(getenv("ADSB_CLI_REGISTER")) == 0);
    const double t_start = now_ms();

    /* start reading before anything touches the GPU */
    ring rg;
    memset(&rg, 0, sizeof rg);
    pthread_t reader;
    int have_reader = 0;
    rg.fd = open(filename, O_RDONLY);
    if (rg.fd >= 0) { /* an unopenable file ends the run silently (air.c:225-228) */
        struct stat sb;
        unsigned long long size = (fstat(rg.fd, &sb) == 0 && sb.st_size > 0) ? (unsigned long long)sb.st_size : 0;
        unsigned long long ring_max = RING_MAX_BYTES;
        if (getenv("ADSB_CLI_RING_MB") && atoll(getenv("ADSB_CLI_RING_MB")) >= 96) /* (measurement knob of this program, not of the library) */
            ring_max = (unsigned long long)atoll(getenv("ADSB_CLI_RING_MB")) << 20;
        if (size > ring_max || size == 0)
            size = ring_max; /* pipes and large files: a bounded ring, the reader waits for free buffers */
        rg.nbuf = (int)(size / buf_bytes) + 2;
        if (rg.nbuf < 3)
            rg.nbuf = 3;
        rg.slot = (ring_slot *)calloc((size_t)rg.nbuf, sizeof *rg.slot);
        pthread_mutex_init(&rg.mu, NULL);
        pthread_cond_init(&rg.cv, NULL);
        have_reader = rg.slot && pthread_create(&reader, NULL, reader_main, &rg) == 0;
    }

    /* -s / -l: the peer first (output.c:277-285: no peer, no packets; an unusable address ends the run with
     * runOutput() == -1).  The file is being read meanwhile. */
    {
        const int prc = sink_wait_peer(&out_sink);
        if (prc == 2) { /* told to end before a peer came */
            adsb_stats z;
            memset(&z, 0, sizeof z);
            print_stats(&z);
            fflush(stderr);
            _exit(0);
        }
        if (prc != 0)
            return 255;
    }

    adsb_config cfg;
    adsb_config_default(&cfg);
    cfg.df18 = df18;
    cfg.fix_1bit = fix1;
    cfg.collect_stats = 1; /* the reference always prints Try/Ok */
    cfg.device = device;   /* (-1: the current one; after the narrowing above, 0) */
    cfg.warm_start = 1;    /* a one-shot process: the runtime's first-use costs are paid inside adsb_create, beside its other work */
    adsb_decoder *dec = adsb_create(&cfg);
    if (!dec) {
        fprintf(stderr, "adsb_create() failed: %s\n", adsb_last_error(NULL));
        return 255; /* runOutput() == -1 -> exit status 255 (main.c:101-105) */
    }
    if (flush && adsb_set_flush(dec, 1) != 0) { /* -E: the stream ends as its silent twin does (and below 2^32 samples: a long stream has no flush) */
        fprintf(stderr, "adsb_set_flush() failed: %s\n", adsb_last_error(dec));
        return 255;
    }
    if (!flush && !iq && !power && adsb_set_long_stream(dec, 1) != 0) { /* always: the reference reads a file of any length (its counter wraps, air.c:34) */
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
                int prc;
                if (power)
                    prc = s->registered ? adsb_push_power_async(dec, (const float *)s->buf, n_samples) : adsb_push_power(dec, (const float *)s->buf, n_samples);
                else if (iq)
                    prc = s->registered ? adsb_push_iq_async(dec, (int)qtype, s->buf, n_samples) : adsb_push_iq(dec, (int)qtype, s->buf, n_samples);
                else if (packed)
                    prc = s->registered ? adsb_push_packed_async(dec, s->buf, n_samples) : adsb_push_packed(dec, s->buf, n_samples);
                else if (converted)
                    prc = s->registered ? adsb_push_async_as(dec, (int)stype, s->buf, n_samples) : adsb_push_as(dec, (int)stype, s->buf, n_samples);
                else
                    prc = s->registered ? adsb_push_async(dec, s->buf, n_samples) : adsb_push(dec, s->buf, n_samples);
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
            if (bytes < buf_bytes)
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
                (unsigned long long)rep.converted, stype == ADSB_FMT_INT16_REAL ? "INT16_REAL" : "FLOAT32_REAL", (unsigned long long)rep.clamped);
    if (iq && qtype == ADSB_FMT_FLOAT32_IQ && adsb_get_format_report(dec, &rep) == 0 && rep.inexact + rep.clamped > 0)
        fprintf(stderr, "%llu of %llu float scalars were rounded to the int16 grid (%llu clamped): expected of a float32 IQ capture\n",
                (unsigned long long)(rep.inexact + rep.clamped), (unsigned long long)rep.converted, (unsigned long long)rep.clamped);
    /* no adsb_destroy / unregister / free: the process ends here, and tearing the GPU runtime
     * down cleanly costs tens of milliseconds that an offline decode has no use for */
    fflush(stderr);
    if (getenv("ADSB_CLI_CLEAN_EXIT")) /* (a profiler's knob: rocprofv3 writes its trace from an exit handler) */
        exit(rc);
    _exit(rc);
}
