/*
 * adsbdec_amd_cli.c -- host program in C for the offline "-f" path, calling the
 * HIP library through the C-ABI of include/adsbdec_amd.h.  This file: the manual, and main() = parse, refuse, dispatch.
 * options.c: the command line and which options go together; common.c: what every mode uses; one file per mode --
 * stream.c (the plain decode), batch.c (-G, -B), export.c (-W), level.c (-L, -I), bursts.c (-U, -K, -P, -k), record.c (-S, -O); cli.h.
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
 *     -S factor[,lead[,hang[,piece]]]  EXTENSION: GATE A STREAM OF ANY LENGTH (adsb_level_windows, adsb_bursts_slice_device).  The uint16 file
 *                   or FIFO of -f is read in pieces of `piece` runs (28 power samples each; default 299 593, about 16 Mi samples); a
 *                   piece is one window call for its report and envelope and one gate call that JOINS BURSTS ACROSS THE PIECES: the
 *                   bursts are those -L -U finds in the whole stream with the same threshold, whatever the piece.  threshold = factor x
 *                   the median of the FIRST piece (adsb_level_percentile at 0.5), fixed for the stream; `@value` in place of the factor is
 *                   the threshold itself.  stdout: once `bursts threshold T lead L hang H`, then `FIRST END HOT PEAK` per burst as it
 *                   closes, in power samples of the stream.  lead and hang default to -U's 2 and 1468 (for -k, hang 4 is enough).  Memory
 *                   is bounded: the device holds the piece and, in front of it, the samples from the open burst's begin on (or the last
 *                   lead runs).  More than 64 Mi samples retained: the gate never closes -- a message that says to raise the factor,
 *                   status 255.  The stream ends at the end of the file or at SIGINT / SIGTERM / SIGQUIT, and what is open is closed
 *                   there; at 2^31 runs (about 100 minutes) it is ended as if the file did: a message, status 255.  A first piece
 *                   without a sign-clear power sample: no threshold, status 255.  uint16 input only (the one flavour with a window
 *                   call): not with -L, -I, -U, -K, -P, -k, -t, -p, -q, -w, -W, -G, -B, -E, -x, -m, -b, -s, -l or several -f.
 *     -O out.brs    EXTENSION, with -S: KEEP ONLY THE BURSTS.  The samples of the bursts a piece closes are gathered on the GPU
 *                   (adsb_gather_device, one call and one copy back per piece) and appended to out.brs.spool; at the end out.brs -- the
 *                   archive -L -U -K writes for the whole stream with that threshold: version 1, kind 4 -- is written as out.brs.tmp
 *                   (header, table, the spool) and renamed, so a run that fails leaves no out.brs; the spool file is removed.  On
 *                   stderr `kept B bursts, X of Y bytes`.  Not without -S.
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
#include "adsbdec_amd.h"
#include "cli.h"

/* A mode returns only where it has failed (main ends with that status, through a normal exit); a run that went its way
 * leaves through cli_exit, without tearing the runtime down. */
int main(int argc, char **argv)
{
    struct cli_options o;
    int rc;
    if ((rc = cli_parse(argc, argv, &o)) != 0 || (rc = cli_refuse(&o)) != 0)
        return rc;
    if (o.listfile)
        return run_batch(&o);
    if (o.record_arg)
        return run_record(&o);
    if (o.level)
        return o.interval_arg ? run_level_windows(&o) : run_level(&o);
    if (o.export_path)
        return run_export(&o);
    install_signals();
    cli_open_sink(&o);
    if (o.archive_in)
        return run_archive(&o);
    if (o.ndev && multi_takes(&o))
        return run_multi(&o);
    if (o.ndev) /* (a single -f that is no readable regular file: streamed through the first device listed) */
        o.device = o.devs[0], o.ndev = 0;
    return run_stream(&o);
}
