/* options.c -- the host program's command line: the usage text, the getopt loop, and which options go together.  Nothing here
 * touches the input file, a peer or the GPU runtime. */
#include "cli.h"

/* (The text is pinned word for word by the recorded grid of tests/test_cli_options_cpu.py; the record mode, -S and -O, came after
 * that recording and is described in the manual at the head of adsbdec_amd_cli.c and by its own refusals.) */
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

/* -t, -q: a whole number, or -1 */
static long parse_type(const char *arg)
{
    char *end;
    const long v = strtol(arg, &end, 10);
    return *end || end == arg ? -1 : v;
}

static int usage_status(void)
{
    usage();
    return 1;
}

int cli_parse(int argc, char **argv, struct cli_options *o)
{
    memset(o, 0, sizeof *o);
    o->device = -1;
    o->burst.lead = 2, o->burst.hang = 1468;
    o->record.lead = 2, o->record.hang = 1468, o->record.piece = 299593;
    o->stype = ADSB_FMT_RAW;
    o->qtype = -1;
    o->outmode = SINK_STDOUT;
    /* the options that only switch something on, and the ones that only name a file */
    static const char switches[] = "axpwLEk", paths[] = "BWKPO";
    int *const on[] = {&o->df18, &o->fix1, &o->packed, &o->power, &o->level, &o->flush, &o->archive_in};
    const char **const path[] = {&o->listfile, &o->export_path, &o->archive_out, &o->pack_out, &o->record_out};
    int c;
    while ((c = getopt(argc, argv, "f:g:ambxpwd:G:s:l:B:t:q:W:LI:U:EK:kP:S:O:")) != EOF) {
        char *end;
        const char *at;
        switch (c) {
        case 'f':
            o->filename = optarg;
            if (o->nfiles == MAX_FILES) /* (more captures than this program keeps track of: say so, do not drop them) */
                return usage_status();
            o->files[o->nfiles++] = optarg;
            break;
        case 'd': {
            const long k = strtol(optarg, &end, 10);
            if (*end || k < 0 || k > 1023)
                return usage_status();
            o->device = (int)k;
            break;
        }
        case 'G':
            o->ndev = parse_gpus(optarg, o->devs);
            if (o->ndev == 0)
                return usage_status();
            break;
        case 's':
        case 'l':
            o->rawaddr = optarg;
            o->outmode = c == 's' ? SINK_CONNECT : SINK_LISTEN;
            break;
        case 'g':
            break;
        case 'm':
        case 'b':
            o->outformat = c == 'm' ? 1 : 2;
            break;
        case 'I':
            o->interval_ms = strtod(optarg, &end);
            if (*end || end == optarg || !(o->interval_ms > 0) || o->interval_ms > 1e12)
                o->interval_ms = 0;
            o->interval_arg = optarg;
            break;
        case 'U': { /* factor[,lead[,hang]]: a finite factor above 0, whole numbers up to 2^30; anything else leaves factor 0 */
            o->burst_arg = optarg;
            o->burst.factor = strtod(optarg, &end);
            int ok = end != optarg && o->burst.factor > 0 && o->burst.factor <= 1.7976931348623157e308;
            uint32_t *field[2] = {&o->burst.lead, &o->burst.hang};
            for (int i = 0; ok && i < 2 && *end == ','; i++) {
                const char *num = end + 1;
                const unsigned long long v = strtoull(num, &end, 10);
                ok = end != num && *num >= '0' && *num <= '9' && v <= (1ull << 30);
                *field[i] = (uint32_t)v;
            }
            if (!ok || *end)
                o->burst.factor = 0;
            break;
        }
        case 'S': { /* factor | @threshold, then [,lead[,hang[,piece]]]: whole numbers, lead and hang up to 2^30, piece 1 .. 2^24 runs */
            const char *num = optarg;
            o->record_arg = optarg;
            o->record.absolute = *num == '@';
            num += o->record.absolute;
            o->record.factor = strtod(num, &end);
            int ok = end != num && o->record.factor > 0 && o->record.factor <= (o->record.absolute ? 3.4028234663852886e38 : 1.7976931348623157e308);
            uint64_t field[3] = {o->record.lead, o->record.hang, o->record.piece};
            for (int i = 0; ok && i < 3 && *end == ','; i++) {
                num = end + 1;
                const unsigned long long v = strtoull(num, &end, 10);
                ok = end != num && *num >= '0' && *num <= '9' && v <= (i < 2 ? 1ull << 30 : 1ull << 24) && (i < 2 || v > 0);
                field[i] = v;
            }
            o->record.lead = (uint32_t)field[0], o->record.hang = (uint32_t)field[1], o->record.piece = field[2];
            if (!ok || *end)
                o->record.factor = 0;
            break;
        }
        case 't':
            o->stype = parse_type(optarg);
            o->stype_arg = optarg;
            break;
        case 'q':
            o->qtype = parse_type(optarg);
            o->qtype_arg = optarg;
            break;
        default:
            if ((at = strchr(switches, c)) != NULL)
                *on[at - switches] = 1;
            else if ((at = strchr(paths, c)) != NULL)
                *path[at - paths] = optarg;
            else
                return usage_status();
        }
    }
    o->converted = o->stype == ADSB_FMT_FLOAT32_REAL || o->stype == ADSB_FMT_INT16_REAL;
    o->iq = o->qtype_arg != NULL;
    return 0;
}

/* One option that a rule's subject does not go with, and why.  The rows of a rule stand in the order of their priority -- the
 * first one present is the one named -- and end with an empty row; rows that share a reason share a line. */
struct clash {
    int present;
    const char *letter, *reason;
};
static int refuse_with(const char *subject, const struct clash *row)
{
    for (; row->letter; row++)
        if (row->present) {
            fprintf(stderr, "%s is not supported with %s: %s\n", subject, row->letter, row->reason);
            return 1;
        }
    return 0;
}
static int refuse(const char *format, const char *arg) /* a message with at most one %s in it */
{
    fprintf(stderr, format, arg);
    return 1;
}

/* Which options go together: every rule turns its run away before any file, peer or GPU call.  The order of the rules among
 * themselves decides which message a line with several clashes gets. */
int cli_refuse(const struct cli_options *o)
{
    const int t = o->stype_arg != NULL, p = o->packed, q = o->iq, w = o->power, E = o->flush, L = o->level, k = o->archive_in;
    const int I = o->interval_arg != NULL, U = o->burst_arg != NULL, K = o->archive_out != NULL, P = o->pack_out != NULL;
    const int G = o->ndev != 0, B = o->listfile != NULL, W = o->export_path != NULL;
    const int s = o->outmode == SINK_CONNECT, l = o->outmode == SINK_LISTEN, several = o->nfiles > 1;
    static const char one_gather[] = "the gather runs on one GPU (-d), one file at a time: no batch and no multi-GPU form";
    static const char no_join[] = "the windows are pieces of a stream, and joining bursts across pieces is the caller's: one file, one call";
    static const char not_both[] = "a run writes the power samples or keeps the capture's bursts, not both";
    static const char multi_reads[] = "the multi-GPU driver reads uint16 and packed files only";
    static const char real_or_iq[] = "a file holds real samples (-t) or IQ samples (-q), not both";
    static const char iq_or_power[] = "a file holds IQ samples (-q) or power samples (-w), not both";
    static const char packed_or_iq[] = "a file is packed 12-bit real or IQ, not both";
    char subject[32];
    const int S = o->record_arg != NULL, O = o->record_out != NULL, x = o->fix1, m = o->outformat == 1, b = o->outformat == 2;

    if (S) { /* -S gates a uint16 stream piece by piece and decodes nothing */
        static const char own_gate[] = "-S reads the stream in pieces and has a level call, a gate and an archive (-O) of its own";
        static const char uint16[] = "the pieces go through adsb_level_windows, which only uint16 samples have";
        static const char one_stream[] = "a stream is recorded on one GPU (-d), one at a time";
        static const char no_packets[] = "a recording decodes nothing: there are no packets to repair, format or send";
        if (refuse_with("-S", (const struct clash[]){
                {L, "-L", own_gate}, {I, "-I", own_gate}, {U, "-U", own_gate}, {K, "-K", own_gate}, {P, "-P", own_gate},
                {k, "-k", "-k reads an archive, -S writes one"},
                {t, "-t", uint16}, {p, "-p", uint16}, {q, "-q", uint16}, {w, "-w", uint16},
                {W, "-W", "a run writes the power samples or records the stream's bursts, not both"},
                {G, "-G", one_stream}, {B, "-B", one_stream},
                {E, "-E", no_packets}, {x, "-x", no_packets}, {m, "-m", no_packets}, {b, "-b", no_packets}, {s, "-s", no_packets},
                {l, "-l", no_packets},
                {several, "several -f", one_stream}, {0}}))
            return 1;
        if (!(o->record.factor > 0))
            return refuse("-S %s: factor[,lead[,hang[,piece]]] -- a finite factor above 0 (or @threshold, a finite float above 0), lead and hang "
                          "whole numbers of runs up to 2^30, piece a whole number of runs from 1 to 2^24\n", o->record_arg);
    }
    if (O && !S)
        return refuse("-O is not supported without -S: it is the archive of the stream that -S gates\n", NULL);

    if (P) { /* -P keeps the pieces -L -U finds of a REAL capture, packed to 12 bits */
        static const char real12[] = "12-bit codes are what a REAL capture carries (a uint16 file, -p or -t 3 | 1); -K keeps IQ and power samples as they are";
        if (!L || !U)
            return refuse("-P is not supported without -L -U: it keeps the bursts that the gate behind the level report finds\n", NULL);
        if (refuse_with("-P", (const struct clash[]){
                {q, "-q", real12}, {w, "-w", real12},
                {K, "-K", "a run writes one archive: the capture's own bytes (-K) or its 12-bit codes (-P)"},
                {I, "-I", no_join},
                {G, "-G", one_gather}, {B, "-B", one_gather},
                {W, "-W", not_both},
                {k, "-k", "-k reads an archive, -P writes one"}, {0}}))
            return 1;
    }
    if (k) { /* -k decodes a burst archive, whose header says what it holds */
        static const char header[] = "the kind of the samples comes from the archive's header";
        static const char one_batch[] = "an archive is decoded on one GPU (-d) by one batch call: no multi-GPU and no list form";
        static const char decoded[] = "the pieces of an archive are decoded, not measured, exported or gathered again";
        if (refuse_with("-k", (const struct clash[]){
                {t, "-t", header}, {p, "-p", header}, {q, "-q", header}, {w, "-w", header},
                {E, "-E", "an archive is always decoded to the last sample of every piece"},
                {G, "-G", one_batch}, {B, "-B", one_batch},
                {L, "-L", decoded}, {W, "-W", decoded}, {K, "-K", decoded},
                {several, "several -f", "one archive at a time"}, {0}}))
            return 1;
    }
    if (K) { /* -K keeps the pieces -L -U finds, out of the capture's own bytes */
        static const char own_bytes[] = "the pieces of a converted or packed capture are not in the capture's own bytes (adsb_gather_device reads those)";
        if (!L || !U)
            return refuse("-K is not supported without -L -U: it keeps the bursts that the gate behind the level report finds\n", NULL);
        if (refuse_with("-K", (const struct clash[]){
                {t, "-t", own_bytes}, {p, "-p", own_bytes},
                {I, "-I", no_join},
                {G, "-G", one_gather}, {B, "-B", one_gather},
                {W, "-W", not_both}, {0}}))
            return 1;
    }
    if (E) { /* -E ends a decode on one GPU past the horizon */
        static const char no_decode[] = "it ends a DECODE at the file's last sample, and this run decodes nothing";
        if (refuse_with("-E", (const struct clash[]){
                {G, "-G", "the multi-GPU driver stitches its shards at the reference's end-of-file horizon; -E decodes on one GPU (-d)"},
                {L, "-L", no_decode}, {W, "-W", no_decode}, {0}}))
            return 1;
    }
    if (L) { /* -L reports the levels of one file in one call and decodes nothing */
        static const char one_level[] = "the level report runs on one GPU (-d), one file at a time: no batch and no multi-GPU form";
        static const char text[] = "the report is text on stdout, not packets for a peer";
        if (refuse_with("-L", (const struct clash[]){
                {G, "-G", one_level}, {B, "-B", one_level},
                {W, "-W", "a run writes the power samples or reports their levels, not both"},
                {s, "-s", text}, {l, "-l", text},
                {several, "several -f", "the report is of one file"}, {0}}))
            return 1;
    }
    if (I) { /* -I cuts -L's report of a uint16 file into windows */
        static const char uint16[] = "the windows are of a uint16 file (adsb_level_windows); a slice of an IQ or power file is already exact on its own";
        if (!L)
            return refuse("-I is not supported without -L: it is the length of the level report's windows\n", NULL);
        if (refuse_with("-I", (const struct clash[]){{t, "-t", uint16}, {p, "-p", uint16}, {q, "-q", uint16}, {w, "-w", uint16}, {0}}))
            return 1;
        if (o->interval_ms == 0)
            return refuse("-I %s: the windows' length in milliseconds, a number above 0\n", o->interval_arg);
    }
    if (U) { /* -U gates the envelope of -L's one call (-L's own refusals, -G, -B and -W among them, stay in front) */
        if (!L)
            return refuse("-U is not supported without -L: it gates the envelope the level report's call writes%s\n",
                          G ? " (and not with -G)" : B ? " (and not with -B)" : W ? " (and not with -W)" : "");
        if (refuse_with("-U", (const struct clash[]){
                {I, "-I", "the windows share one envelope piece by piece, and joining bursts across pieces is the caller's"}, {0}}))
            return 1;
        if (!(o->burst.factor > 0))
            return refuse("-U %s: factor[,lead[,hang]] -- a finite factor above 0, lead and hang whole numbers of runs up to 2^30\n", o->burst_arg);
    }
    if (q && o->qtype == ADSB_FMT_INT8_IQ) { /* int8 IQ is decoded from one file on one GPU and nothing else */
        static const char no_int8[] = "the export reads uint16 codes, int16 IQ (-q 2) or float32 IQ (-q 0); an int8 sample's power is 256 (I^2 + Q^2)";
        /* (-G and -B give -w's or -W's reason where one of those is on the line too: the message has always read so) */
        const char *multi = w ? iq_or_power : W ? no_int8 : multi_reads;
        if (refuse_with("-q 8", (const struct clash[]){
                {t, "-t", real_or_iq},
                {p, "-p", packed_or_iq},
                {G, "-G", multi}, {B, "-B", multi},
                {w, "-w", iq_or_power},
                {W, "-W", no_int8}, {0}}))
            return 1;
    }
    if (W) { /* -W writes power samples and decodes nothing */
        static const char one_export[] = "the export runs on one GPU (-d), one file at a time";
        static const char to_file[] = "power samples go to the file named, not to a peer";
        if (refuse_with("-W", (const struct clash[]){
                {w, "-w", "a file of power samples is already what -W writes"},
                {t, "-t", "the export reads uint16 codes (or IQ samples with -q); python -m adsbdec_amd.sample_formats converts other real types"},
                {p, "-p", "the export reads uint16 codes (or IQ samples with -q); python -m adsbdec_amd.packed12 unpacks"},
                {G, "-G", one_export}, {B, "-B", one_export},
                {s, "-s", to_file}, {l, "-l", to_file},
                {several, "several -f", "the export writes one file"}, {0}}))
            return 1;
    }
    if (t && !o->converted && o->stype != ADSB_FMT_UINT16_REAL && o->stype != ADSB_FMT_RAW) {
        if (o->stype == 0 || o->stype == 2)
            fprintf(stderr, "-t %ld (%s) is not a real sample type: libairspy has already mixed, filtered and decimated an IQ stream, so it has no "
                            "raw twin to be decoded as; -t takes 1 (float32 real), 3 (int16 real), 4 or 5 (uint16)\n",
                    o->stype, o->stype == 0 ? "FLOAT32_IQ" : "INT16_IQ");
        else
            fprintf(stderr, "-t %s: unknown sample type; -t takes 1 (float32 real), 3 (int16 real), 4 or 5 (uint16)\n", o->stype_arg);
        return 1;
    }
    snprintf(subject, sizeof subject, "-t %ld", o->stype);
    if (o->converted && refuse_with(subject, (const struct clash[]){
            {p, "-p", "a file is packed 12-bit or of that type, not both"},
            {G, "-G", multi_reads}, {B, "-B", multi_reads}, {0}}))
        return 1;
    if (q && o->qtype != ADSB_FMT_INT16_IQ && o->qtype != ADSB_FMT_FLOAT32_IQ && o->qtype != ADSB_FMT_INT8_IQ)
        return refuse("-q %s: not an IQ sample type; -q takes 2 (int16 IQ), 0 (float32 IQ) or 8 (int8 IQ), real samples go with -t\n", o->qtype_arg);
    snprintf(subject, sizeof subject, "-q %ld", o->qtype);
    if (q && refuse_with(subject, (const struct clash[]){
            {t, "-t", real_or_iq},
            {p, "-p", packed_or_iq},
            {G, "-G", multi_reads}, {B, "-B", multi_reads}, {0}}))
        return 1;
    if (w && refuse_with("-w", (const struct clash[]){
            {t, "-t", "a file holds real samples (-t) or power samples (-w), not both"},
            {q, "-q", iq_or_power},
            {p, "-p", "a file is packed 12-bit real or float32 power, not both"},
            {G, "-G", multi_reads}, {B, "-B", multi_reads}, {0}}))
        return 1;
    if (B) /* a batch: its own inputs and outputs -- no -f, no peer; -d and -G exclude each other here too */
        return o->filename || s || l || (G && o->device >= 0) ? usage_status() : 0;
    /* several captures need -G and go to files; -d and -G exclude each other */
    if (!o->filename || (several && (!G || s || l)) || (G && o->device >= 0))
        return usage_status();
    if (p && G) /* (every mode but the plain decode has refused -G above) */
        return refuse("-p (packed 12-bit input) is not supported with -G: the multi-GPU driver reads uint16 files only\n", NULL);
    return 0;
}
