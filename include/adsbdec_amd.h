/* adsbdec_amd.h -- C-ABI of libadsbdec_amd.so: the MI355X (gfx950) drop-in for the offline "-f" demodulation path of TLeconte/adsbdec.
 * Everything a drop-in host and a multi-GPU host call; the primitives underneath and the test knobs are in adsbdec_amd_diag.h.  The
 * reference has no plugin/FFI interface: one prototype (adsbdec.h:5) plus extern C functions with file-scope state (SURVEY.md 8b).  Each entry point names the reference seam it stands behind (file:line); INTEGRATION.md shows the change in air.c / output.c that binds them.
 * Conventions follow the reference: int 0 / -1 with a message from adsb_last_error() (air.c:113-118 prints to stderr); one producer thread
 * per handle (decodeiq is not re-entrant: air.c:33-34,49-50, demod.c:86); plain pointers and sizes.  HIP is the only implementation: no CPU fallback; adsb_create() fails loudly when no gfx950 device is usable.
 * Input domain.  uint16 samples carrying the Airspy's 12-bit ADC code centred on 2048 (air.c:64).  Bit-identical to the reference for every
 * code in [0, 4095] and up to |x-2048| <= ~23 000; beyond, the reference's `int p1 = float + float` (demod.c:102-105) overflows while this
 * library compares un-wrapped values: accepted, no parity claimed (SURVEY Q1).  Streams end below 2^32 samples (the reference's `fidx` wraps there, SURVEY Q13: a push that would reach it fails) unless adsb_set_long_stream is on: any length, decoded as the reference does (DESIGN.md). */
#ifndef ADSBDEC_AMD_H
#define ADSBDEC_AMD_H
#include <stddef.h>
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
/* Bumped when an entry point or struct member changes meaning or place; within one version adsb_config and adsb_profile grow at their END only. */
#define ADSB_ABI_VERSION 5
#define ADSB_PULSEW 5 /* constants of the path (adsbdec.h:1-3, air.c:32,47) */
#define ADSB_DECOFFSET 1200
#define ADSB_APBUFFSZ 40980
#define ADSB_WINDOW 1196 /* power samples one long-frame evaluation touches: a[g .. g+1195] */
typedef struct adsb_decoder adsb_decoder; /* one stream == the statics of air.c / demod.c / valid.c */
/* Record leaving the path == netout()'s arguments (valid.c:26, output.c:159) == blk_t (output.c:45-52), plus the preamble's global index. */
typedef struct adsb_frame {
    uint64_t g;        /* global 10 MS/s power-sample index of the preamble start */
    uint64_t ts;       /* demod.c:86,99: loop-pass counter at acceptance          */
    uint32_t pw;       /* demod.c:127,133: (p1+p2)/4                              */
    uint8_t len;       /* 7 (DF11) or 14 (DF17/18)                                */
    uint8_t frame[14]; /* demod.c:110-123                                         */
    uint8_t reserved;  /* bit 0: repaired by the 1-bit extension (cfg.fix_1bit)   */
} adsb_frame;
typedef struct adsb_stats { /* valid.c:30-31,84-100: Try/Ok per DF, in the order 11, 17, 18 */
    uint64_t try_[3];
    uint64_t ok[3];
    uint64_t fixed; /* frames accepted after a 1-bit repair (extension; 0 by default) */
} adsb_stats;
typedef struct adsb_config {
    uint32_t struct_size;   /* sizeof(adsb_config) as the CALLER knows it                                         */
    uint32_t abi;           /* ADSB_ABI_VERSION of the caller's header; anything else is refused                  */
    int32_t df18;           /* demod.c:26 `df`, set by -a (main.c:76-78)                                          */
    int32_t device;         /* HIP device ordinal; -1 = the current device                                        */
    int32_t collect_stats;  /* reproduce valid.c's Try counters (the reference always does; costs a try list)     */
    int32_t profile;        /* time every scan launch on the device's own 100 MHz clock: adsb_profile.kernel_ms   */
    uint64_t stage_samples; /* device staging capacity for adsb_push(); 0 = default (32 Mi)                       */
    void *stream;           /* hipStream_t to launch on; NULL = a stream owned by the handle                      */
    int32_t all_candidates; /* 1: the device reports EVERY CRC-valid offset; 0 (default): not those the greedy scan can never visit (same frames) */
    int32_t fix_1bit;       /* EXTENSION (SURVEY Q8), off by default: repair DF17/18 frames whose CRC residual is the syndrome of one bit in [5,112) */
    int32_t push_overlap;   /* 1: adsb_push() returns once `samples` is COPIED, the scan in flight; its frames drain one call later (INTEGRATION.md) */
    int32_t host_threads;   /* Threads that consume the hand-off stream.  1: the caller alone, ALWAYS.  2: + a reader thread; N >= 3 (<= 17): + N - 2 that
                               decide tiles ahead.  0 (default): 1, then 6 (2 below 12 CPUs) under dense traffic (INTEGRATION.md).  Same frames always. */
    int32_t wait_timeout_s; /* no wait for the device lasts longer (0 = default, 120 s): then -1, adsb_last_error() names what was waited for */
    int32_t warm_start;     /* 1: adsb_create also pays the runtime's first-use costs of copying (7-9 ms each): for a one-shot process */
    const void *debug;      /* NULL, or an adsb_debug_config (adsbdec_amd_diag.h: test knobs); copied by adsb_create */
} adsb_config;
/* Counters accumulate over the life of the handle (adsb_reset keeps them: take differences); the last three members came with ABI 5. */
typedef struct adsb_profile {
    uint64_t launches;     /* scan-kernel launches since adsb_create                                  */
    uint64_t relaunches;   /* launches repeated after a record-buffer overflow                        */
    uint64_t offsets;      /* preamble offsets those launches covered                                 */
    double kernel_ms;      /* sum of their durations on the device clock (profile=1 only)             */
    double last_kernel_ms;
    uint64_t last_offsets;
    uint64_t candidates;   /* CRC-valid candidates received from the device                           */
    uint64_t tries;        /* DF-gate passes that came through launch-wide lists (collect_stats=1)    */
    double host_ms;        /* host time spent checking + resolving records                            */
    double wait_ms;        /* host time blocked waiting for the device                                */
    uint64_t big_offsets;  /* offsets per launch of the largest launch size seen                      */
    uint64_t big_launches; /* launches of that size                                                   */
    double big_ms;         /* sum of their durations on the device clock (profile=1)                  */
    uint32_t host_threads_running; /* the handle's own threads that exist NOW: reader (0/1) + gang helpers; 0 under ordinary traffic */
    uint32_t gang_launches;        /* launches whose frames went through the gang                                  */
    uint64_t gang_batches;         /* batches of tiles handed to the gang to be decided ahead of the caller        */
} adsb_profile;
/* Defaults; the struct's size is the CALLER's: adsb_config_default(&cfg) = adsb_config_init(&cfg, sizeof cfg), which sets cfg.abi. */
void adsb_config_init(adsb_config *cfg, size_t struct_size);
#define adsb_config_default(cfg) adsb_config_init((cfg), sizeof(adsb_config))
/* The stream state that air.c:33-34,49-50 / demod.c:86 / valid.c:30-31 keep in statics.  NULL on failure
 * (adsb_last_error(NULL) has the reason).  adsb_reset: the same handle, a fresh stream (ring, ts, stats). */
adsb_decoder *adsb_create(const adsb_config *cfg);
void adsb_destroy(adsb_decoder *d); int adsb_reset(adsb_decoder *d);
/* Sample ingress; replaces `decodeiq(const unsigned short *r, const int len)` (air.c:54), called from fileInput (air.c:239) / rx_callback
 * (air.c:175).  `samples` is borrowed for the call.  Any n: the stream is the concatenation of all pushes (the reference needs n % 4 == 0). */
int adsb_push(adsb_decoder *d, const uint16_t *samples, size_t n);
/* From a double-buffered read loop (INTEGRATION.md): returns once copy and scan are ENQUEUED; `samples` stays borrowed until the next push / finish / sync; adsb_sync waits for all. */
int adsb_push_async(adsb_decoder *d, const uint16_t *samples, size_t n); int adsb_sync(adsb_decoder *d);
/* Samples already in HBM: scanned in place when 16-byte aligned at a stream position that is a multiple of 8 samples.  _final = push of the LAST piece + adsb_finish. */
int adsb_push_device(adsb_decoder *d, const void *device_samples, size_t n); int adsb_push_device_final(adsb_decoder *d, const void *device_samples, size_t n);
/* `adsbdec -f` for ONE capture in HBM: adsb_reset + adsb_push_device_final + adsb_take.  The number of frames (*frames as adsb_take) or -1. */
long adsb_decode_device(adsb_decoder *d, const void *device_samples, size_t n, const adsb_frame **frames);
/* n_captures INDEPENDENT captures in as few launches as they fit, each decoded as adsb_decode_device(d, p[i], n[i]) would decode it alone, and
 * the handle left as by that call.  Capture i's frames are (*frames)[first[i] .. first[i+1]) (first: n_captures + 1 entries), valid as adsb_take's;
 * stats: NULL, or n_captures tables.  Returns all frames' number, or -1, handle unchanged: a _device pointer not 16-byte aligned, n[i] >= 2^32. */
long adsb_decode_batch_device(adsb_decoder *d, size_t n_captures, const void *const *device_samples, const size_t *n,
                              const adsb_frame **frames, uint64_t *first, adsb_stats *stats);
long adsb_decode_batch_host(adsb_decoder *d, size_t n_captures, const uint16_t *const *samples, const size_t *n,
                            const adsb_frame **frames, uint64_t *first, adsb_stats *stats);
/* Airspy packed 12-bit input (air.c:120,128,150-151,173-177).  A group is 8 samples s0..s7 (12-bit codes, air.c:64) in three little-endian 32-bit
 * words w0 w1 w2; as ONE 96-bit big-endian number w0:w1:w2 it is s0 .. s7, most significant first (from this definition, not checked against libairspy):
 *   s0 = w0 >> 20,  s1 = (w0 >> 8) & 0xfff,  s2 = (w0 & 0xff) << 4 | w1 >> 28,  s3 = (w1 >> 16) & 0xfff,  s4 = (w1 >> 4) & 0xfff,
 *   s5 = (w1 & 0xf) << 8 | w2 >> 24,  s6 = (w2 >> 12) & 0xfff,  s7 = w2 & 0xfff.
 * n counts SAMPLES: n % 8 == 0, ADSB_PACKED12_BYTES(n) bytes are read, at a stream position that is a multiple of 8 (uint16 and packed pushes mix
 * there); device pointers 4-byte aligned.  Otherwise -1, handle unchanged.  Frames, ts, Try/Ok, counters and contracts: the uint16 calls'.  Extra device memory the handle keeps (grown on demand): host pushes, two landing buffers of 1.5 B x stage_samples; device pushes, a scratch of 2 B x n. */
#define ADSB_PACKED12_BYTES(n) ((n) / 8 * 12)
int adsb_push_packed(adsb_decoder *d, const void *packed, size_t n); int adsb_push_packed_async(adsb_decoder *d, const void *packed, size_t n);
int adsb_push_device_packed(adsb_decoder *d, const void *device_packed, size_t n); int adsb_push_device_packed_final(adsb_decoder *d, const void *device_packed, size_t n);
long adsb_decode_device_packed(adsb_decoder *d, const void *device_packed, size_t n, const adsb_frame **frames);
/* adsb_decode_batch_device / _host for packed captures (n[i] counts samples): results, first / stats and the handle's state as theirs, capture i
 * decoded as its unpacked twin alone.  Refused by capture index, handle unchanged: n[i] % 8 != 0, a _device pointer not 4-byte aligned, NULL with n[i] > 0, n[i] >= 2^32.  Extra device memory: a scratch of 2 B x sum n (captures at 128-byte boundaries), ONE launch; _host: + 1.5 B x sum n. */
long adsb_decode_batch_device_packed(adsb_decoder *d, size_t n_captures, const void *const *device_packed, const size_t *n,
                                     const adsb_frame **frames, uint64_t *first, adsb_stats *stats);
long adsb_decode_batch_host_packed(adsb_decoder *d, size_t n_captures, const void *const *packed, const size_t *n,
                                   const adsb_frame **frames, uint64_t *first, adsb_stats *stats);
/* Other REAL sample formats, converted to the uint16 code on the GPU; fmt is the airspy_rx -t number (from the definitions below, not checked against
 * libairspy).  3 INT16_REAL: int16 x = (code - 2048) << 4; code = (x >> 4) + 2048; inexact iff x & 15.  1 FLOAT32_REAL: x = (code - 2048) / 2048;
 * r = rint(2048 x), code = r + 2048 clamped to [0, 4095] -- clamped: outside, +-Inf, NaN (-> 2048); else inexact iff (code - 2048) / 2048 is not x (every denormal is, -0.0 is not).  4 UINT16_REAL, 5 RAW: the uint16 call of the same kind and its rules.  0, 2 (IQ: no raw twin), anything else: -1.
 * Any n at any stream position, mixing with the other pushes; device pointers aligned to the element, else -1, handle unchanged.  Frames, ts, Try/Ok
 * and contracts: the uint16 calls'.  Extra device memory, kept as for packed input: host pushes, two landing buffers of (2 or 4) B x stage_samples; device pushes and batches, the packed calls' scratch (2 B x n; ONE conversion launch per batch); _batch_host: + (2 or 4) B x sum n. */
enum { ADSB_FMT_FLOAT32_REAL = 1, ADSB_FMT_INT16_REAL = 3, ADSB_FMT_UINT16_REAL = 4, ADSB_FMT_RAW = 5 }; size_t adsb_format_bytes(int fmt, size_t n); /* bytes of n samples (0: a format that is refused) */
int adsb_push_as(adsb_decoder *d, int fmt, const void *samples, size_t n); int adsb_push_async_as(adsb_decoder *d, int fmt, const void *samples, size_t n);
int adsb_push_device_as(adsb_decoder *d, int fmt, const void *device_samples, size_t n); int adsb_push_device_final_as(adsb_decoder *d, int fmt, const void *device_samples, size_t n);
long adsb_decode_device_as(adsb_decoder *d, int fmt, const void *device_samples, size_t n, const adsb_frame **frames);
long adsb_decode_batch_device_as(adsb_decoder *d, int fmt, size_t n_captures, const void *const *device_samples, const size_t *n,
                                 const adsb_frame **frames, uint64_t *first, adsb_stats *stats);
long adsb_decode_batch_host_as(adsb_decoder *d, int fmt, size_t n_captures, const void *const *samples, const size_t *n,
                               const adsb_frame **frames, uint64_t *first, adsb_stats *stats);
/* Since adsb_create / adsb_reset: samples converted, and those off their format's grid (a wrong fmt shows here).  Waits for the conversions enqueued. */
typedef struct adsb_format_report { uint64_t converted, inexact, clamped; } adsb_format_report;
int adsb_get_format_report(const adsb_decoder *d, adsb_format_report *out);
/* COMPLEX captures at 10 MS/s: airspy_rx -t 2 INT16_IQ (its default) and -t 0 FLOAT32_IQ.  libairspy has already mixed, filtered and decimated them: no raw
 * twin (the _as calls refuse 0 and 2), but they ARE where demod.c works: power sample a[m] = |sample m|^2, everything behind it the reference's code on that array.
 * INT16_IQ: little-endian int16 (I, Q); i = I / 16, q = Q / 16, a = fl(fl(i i) + fl(q q)), binary32, nothing fused.  The / 16 puts I, Q in ADC-code units like
 * (float)r - 2048: demod.c:102-105's int truncation acts at its granularity; pw and the Beast level are on a COMPARABLE scale, not a calibrated one (nobody here
 * has measured libairspy's filter gain).  FLOAT32_IQ: binary32 (I, Q), nominal [-1, 1); each scalar r = rint(32768 x), ties to even, clamped to [-32768, 32767] (NaN -> 0, +-Inf clamped), then as INT16_IQ: 1/16 ADC LSB.  libairspy's float path need not sit on that grid: expect adsb_get_format_report's inexact (per
 * scalar) to be non-zero for real -t 0 files.  Power samples enter in twos (air.c:94-99): a trailing odd sample at adsb_finish is never seen.  n counts COMPLEX
 * samples.  A stream's kind, real or IQ, is fixed by its first push with samples after adsb_create / adsb_reset; the other kind then returns -1.  Also refused, handle unchanged: fmt not 0 / 2, NULL with n > 0, a device pointer not 4-byte aligned, a stream reaching 2^31 complex samples, an adsb_set_long_stream handle.
 * fmt 2 device pointers: in place when 16-byte aligned at a multiple of 4 complex samples, else staged; fmt 0: converted on the GPU (FLOAT32_REAL's buffers).  INT8_IQ = 8 is NOT an airspy_rx -t number (the name means "8 bits"): interleaved signed bytes I, Q, two per complex sample at 10 MS/s -- hackrf_transfer's cs8, bladeRF / USRP sc8.  Decoded exactly as fmt 2 decodes the widened twin (I << 8, Q << 8): a[m] = 256 (I^2 + Q^2), an integer <= 2^23, exact in binary32; never converted, so adsb_get_format_report says (0, 0, 0).  A stream kind of its own: fmt 8 does not mix with fmt 0 / 2, real or power pushes (-1, both named).  Refused like fmt 2, but the device pointer must be 2-byte aligned; in place under fmt 2's rule (16-byte aligned at a multiple of 4 complex samples: the kernel's lanes are then 8-byte aligned, its 4-byte loads ask for less), anything else staged.  Not exported (adsb_power_device_iq), not sharded. */
enum { ADSB_FMT_FLOAT32_IQ = 0, ADSB_FMT_INT16_IQ = 2, ADSB_FMT_INT8_IQ = 8 }; size_t adsb_iq_bytes(int fmt, size_t n); /* bytes of n complex samples: 8 n, 4 n, 2 n; 0 for anything else */
int adsb_push_iq(adsb_decoder *d, int fmt, const void *samples, size_t n); int adsb_push_iq_async(adsb_decoder *d, int fmt, const void *samples, size_t n);
int adsb_push_device_iq(adsb_decoder *d, int fmt, const void *device_samples, size_t n); int adsb_push_device_iq_final(adsb_decoder *d, int fmt, const void *device_samples, size_t n);
long adsb_decode_device_iq(adsb_decoder *d, int fmt, const void *device_samples, size_t n, const adsb_frame **frames);
long adsb_decode_batch_device_iq(adsb_decoder *d, int fmt, size_t n_captures, const void *const *device_samples, const size_t *n,
                                 const adsb_frame **frames, uint64_t *first, adsb_stats *stats);
long adsb_decode_batch_host_iq(adsb_decoder *d, int fmt, size_t n_captures, const void *const *samples, const size_t *n,
                               const adsb_frame **frames, uint64_t *first, adsb_stats *stats);
/* float32 POWER samples at 10 MS/s: a[0:n] IS the reference's ampbuff stream (adsbdec.h:5 deqframe(const float *ampbuff, const int len)), from any front end.  Decoded exactly as
 * the _iq calls decode a[] behind their squaring step: samples enter in twos (air.c:94-99), a trailing odd one at adsb_finish is never seen, the EOF horizon is the reference's with
 * M = n - (n & 1); pw = ((int)(a[g] + a[g+10]) + (int)(a[g+35] + a[g+45])) / 4 (demod.c:102-105,127,133); a sample outside the buffer reads as +0.  INPUT DOMAIN: every sample finite,
 * sign bit clear, below 2^29 (no negatives, -0.0, NaN, Inf; subnormals are inside): the reference's int sums then stay below 2^31.  Outside it nothing is promised; adsb_level_device_power detects it (negative, hist[1248 ..]).  n counts power samples.
 * A third stream kind beside real and IQ (fixed by the first push with samples; another kind then returns -1).  Also refused, handle unchanged: NULL with n > 0, a device pointer not
 * 4-byte aligned, a stream reaching 2^31 power samples, an adsb_set_long_stream handle.  Device pointers: in place when 16-byte aligned at a multiple of 4 samples, else staged. */
int adsb_push_power(adsb_decoder *d, const float *samples, size_t n); int adsb_push_power_async(adsb_decoder *d, const float *samples, size_t n);
int adsb_push_device_power(adsb_decoder *d, const void *device_samples, size_t n); int adsb_push_device_power_final(adsb_decoder *d, const void *device_samples, size_t n);
long adsb_decode_device_power(adsb_decoder *d, const void *device_samples, size_t n, const adsb_frame **frames);
long adsb_decode_batch_device_power(adsb_decoder *d, size_t n_captures, const void *const *device_samples, const size_t *n, const adsb_frame **frames, uint64_t *first, adsb_stats *stats);
long adsb_decode_batch_host_power(adsb_decoder *d, size_t n_captures, const float *const *samples, const size_t *n, const adsb_frame **frames, uint64_t *first, adsb_stats *stats);
/* The way OUT at that boundary: the reference's ampbuff (air.c:54-91), bit for bit, in an array of the caller's.  adsb_power_window: the buffer holds uint16 samples
 * [first_sample, first_sample + n) of a stream; power[i] = power sample m_begin + i.  RULES (one by one in INTEGRATION.md); one broken: -1, a message, nothing written.
 *   1. first_sample % 8 == 0; device_samples and device_power 16-byte aligned; m_begin % 28 == 0; m_begin <= m_end; power_cap >= m_end - m_begin.
 *   2. Every sample's OWN pair is held: 2 m_begin >= first_sample, 2 m_end <= first_sample + n.  The six OLDER pairs read as silence (0x800) if not held.
 *   3. first_sample + n < 2^32, on adsb_set_long_stream handles too.  4. Returns m_end - m_begin, every float written; an empty window launches nothing.
 *   5. The handle's stream and resolver stay untouched: callable between pushes.  6. _as and _iq (fmt 0) add to adsb_get_format_report.
 * _host: through buffers the handle keeps.  adsb_power_device: the window (0, n, 0, 2 (n / 4)).  _as (fmt 1 | 3) / _packed: through the scratch of
 * adsb_decode_device_as / _packed, shared with them.  _iq (fmt 2 | 0): n COMPLEX samples -> n power samples.  adsb_power_batch_*: a BATCH of captures, capture i exactly as the single call of the same flavour exports it alone (the same floats from device_power[i][0] on; a fresh stream each: the six pairs before its first sample read as silence, never as a neighbour's samples), in ONE export launch behind at most one unpack (_packed) or conversion (_as fmt 1 | 3, _iq fmt 0) launch into the scratch of adsb_decode_batch_device_packed / _as; returns the floats written in all; rules 5 and 6 hold.  Refused (-1, the message names the capture, nothing launched, written or counted; INTEGRATION.md): what the single call refuses of a capture, n[i] >= 2^32 (IQ: 2^31), power_cap[i] below its count, n_captures >= 2^32 - 1.  A capture without power samples (n[i] < 4; IQ: 0) may have NULL pointers and costs nothing.
 * adsb_level_*: HOW LOUD a capture is, in one pass that stores almost nothing: the report of exactly the M floats a[] that the export call of the same flavour writes (_iq takes fmt 8 too: a = 256 (I^2 + Q^2); _power: the caller's floats), b = their bit patterns.  negative: samples with the sign bit set (-0.0 counts); hist[k]: sign-clear samples with b >> 20 == k (8 bins per octave, 0.75 dB; 1.0 is bin 1016, 2^29 is 1248, Inf / NaN 2040 and up; sum + negative == samples; the _power domain holds iff negative == 0 and hist[1248 ..] == 0); rail_lo / rail_hi / over: input codes == 0 / == 4095 / > 4095 over EVERY sample of the capture, the trailing n % 4 too (real; _as / _packed: of the converted codes), scalars == -32768 / 32767 (IQ fmt 2, and 0 behind its conversion: a clamped float shows) or -128 / 127 (fmt 8), over 0; all 0 for _power.  device_env: NULL with env_cap 0, or env_cap >= ceil(M / 28) floats, 4-byte aligned: env[r] = the float whose bits are the unsigned maximum of (b, sign clear, else 0) over samples [28 r, 28 r + 28) -- in the domain the run's maximum.  Returns M (0: a zeroed report, nothing launched) or -1, nothing written, not the format report either; pointers and lengths as the export call of the flavour (fmt 8: 2-byte aligned, n < 2^31); export rules 5 and 6 hold.  adsb_level_batch_*: a BATCH of captures, capture i exactly the report -- and, where device_env[i] is given, the envelope -- that the single call of the same flavour gives for it alone (a fresh stream each: the six pairs before its first sample read as silence, never as a neighbour's samples; the rail counters over every code of the capture, its trailing n % 4 too); out: n_captures reports in host memory; device_env and env_cap both NULL (no envelope at all), or per capture the single call's NULL with 0 / ceil(M_i / 28) floats.  Up to 1024 captures share ONE level launch behind at most one unpack (_packed) or conversion (_as fmt 1 | 3, _iq fmt 0) launch into the scratch of adsb_decode_batch_device_packed / _as, one memset and one copy back of their totals (16 KiB a capture: 16 MiB of device and of pinned memory, kept by the handle); larger batches go in such sub-batches.  Returns the sum of the M_i; export rules 5 and 6 hold.  Refused (-1, the message names the capture, nothing launched, written or counted; INTEGRATION.md): what the single call refuses of a capture, n[i] >= 2^32 (IQ, fmt 8 and _power: 2^31), NULL arrays or out, n_captures >= 2^32 - 1.  A capture without power samples (n[i] < 4; IQ and _power: 0) gets a zeroed report, may have NULL pointers and costs nothing.  adsb_level_windows: ONE stream, n_windows consecutive WINDOWS of it in one launch per 1024 -- the buffer holds uint16 samples [first_sample, first_sample + n) as adsb_power_window's does (rules 1 to 3 and 5), edges[0] <= ... <= edges[n_windows] are power samples of the stream, every edge but the last a multiple of 28; out[i] = the report of the floats adsb_power_window writes for [edges[i], edges[i + 1]) (the six older pairs from the buffer where it holds them, else silence) with the rail counters of the codes of their OWN pairs, samples 2 edges[i] .. 2 edges[i + 1]; an empty window: a zeroed report.  The reports add (adsb_level_add: *sum += *part, no device) to the report of [edges[0], edges[n_windows]).  This is where ONE window over a whole capture differs from adsb_level_device: a stream's trailing n % 4 codes belong to no window, so the rails leave them out.  device_env: NULL with 0, or ceil((edges[n_windows] - edges[0]) / 28) floats for ALL windows, env[r] the run at power sample edges[0] + 28 r.  Returns edges[n_windows] - edges[0] (n_windows == 0: 0, nothing launched).  Refused (-1, the message names the window, nothing launched, written or counted): a broken rule, an inner edge off 28, descending edges, 2 edges[0] < first_sample, 2 edges[n_windows] > first_sample + n, NULL edges or out, NULL samples with a non-empty span, the envelope's rules, n_windows >= 2^32 - 1.  _host: through buffers the handle keeps.  No multi-GPU or stream-window form of the batch, _as, _packed, _iq and _power calls (INTEGRATION.md).  adsb_level_percentile: no device; the lower edge of the bin that holds the q-quantile of the sign-clear samples (the first bin at which the running count reaches ceil(q total), and 1); -1 on NULL, an empty histogram or q outside [0, 1].  adsb_bursts_*: THE GATE behind the envelope -- env: n_env floats, the envelope a level call wrote or the caller's own; u[r] = the bits of env[r], 0 where its sign is set; run r is HOT iff u[r] >= bits(threshold) as unsigned integers (NaN and Inf are hot, +0.0 makes every run hot); the hot runs, cut wherever two neighbours differ by more than lead + hang + 1, are the bursts: begin = max(0, first - lead), end = min(n_env, last + hang + 1), hot = the hot runs, peak = the float of the largest u among them; ascending, at least one run apart; in power samples [28 begin, min(28 end, M)).  Returns B, the number of bursts, which may exceed cap: the first min(B, cap) records are written to bursts (HOST memory), complete and in order, nothing at or behind bursts[cap]; NULL with cap 0 only counts; n_env 0: 0, nothing launched.  Waits for its kernels; export rule 5 holds.  Refused (-1, nothing launched or written): NULL env with n_env > 0, a pointer off 4 bytes, n_env >= 2^31, a threshold that is NaN or has its sign set, lead or hang above 2^30, a NULL table with cap > 0.  No batch form, no multi-GPU form.  A stream that comes in slices: a burst with begin == 0 or end == n_env touches the edge, and its record no longer says where its hot runs lay, so the tables of slices cannot be joined; adsb_bursts_slice_* gate a slice with what the slices before it left open.  adsb_bursts_slice_*: THE GATE OF A SLICE OF A STREAM -- the stream's runs count from 0; in: a zeroed carry at the start of a stream, then the carry the call before wrote (runs: the runs covered so far; open: a cluster is open, with its first and last hot run, hot count and peak).  The hot runs of the slice, as stream runs, behind the open cluster's, are cut into clusters wherever two neighbours differ by more than join = lead + hang + 1 (this call's); a cluster with last hot run e is CLOSED iff final or e + join < in->runs + n_env (no run still to come can join it) and is then the record begin = max(0, first - lead), end = min(in->runs + n_env, last + hang + 1), hot, peak in STREAM runs; at most one cluster, the last, stays open and goes to *out, out->runs = in->runs + n_env.  The records of consecutive calls with one threshold, lead and hang, the last one final, are adsb_bursts_* of the whole envelope, however it is cut (slices of 0 runs too).  Returns the bursts closed, which may exceed cap: the first min(B, cap) are written (HOST memory), nothing at or behind bursts[cap]; *out is written in full whatever the cap (after B > cap: the same call again with the same in); in == out is allowed; n_env 0 launches nothing (final: closes the carried cluster).  One set of launches on the handle's stream, waited for; export rule 5 holds.  Refused (-1, nothing launched or written): what adsb_bursts_* refuse, a NULL in or out, in->runs + n_env >= 2^31, an open carry that is not first <= last < runs with hot >= 1. */
long adsb_power_window(adsb_decoder *d, const void *device_samples, uint64_t first_sample, size_t n, uint64_t m_begin, uint64_t m_end, float *device_power, size_t power_cap);
long adsb_power_window_host(adsb_decoder *d, const uint16_t *samples, uint64_t first_sample, size_t n, uint64_t m_begin, uint64_t m_end, float *power, size_t power_cap); long adsb_power_batch_host(adsb_decoder *d, size_t n_captures, const uint16_t *const *samples, const size_t *n, float *const *power, const size_t *power_cap);
long adsb_power_device(adsb_decoder *d, const void *device_samples, size_t n, float *device_power, size_t power_cap); long adsb_power_batch_device(adsb_decoder *d, size_t n_captures, const void *const *device_samples, const size_t *n, float *const *device_power, const size_t *power_cap);
long adsb_power_device_as(adsb_decoder *d, int fmt, const void *device_samples, size_t n, float *device_power, size_t power_cap); long adsb_power_batch_device_as(adsb_decoder *d, int fmt, size_t n_captures, const void *const *device_samples, const size_t *n, float *const *device_power, const size_t *power_cap);
long adsb_power_device_packed(adsb_decoder *d, const void *device_packed, size_t n, float *device_power, size_t power_cap); long adsb_power_batch_device_packed(adsb_decoder *d, size_t n_captures, const void *const *device_packed, const size_t *n, float *const *device_power, const size_t *power_cap);
long adsb_power_device_iq(adsb_decoder *d, int fmt, const void *device_samples, size_t n, float *device_power, size_t power_cap); long adsb_power_batch_device_iq(adsb_decoder *d, int fmt, size_t n_captures, const void *const *device_samples, const size_t *n, float *const *device_power, const size_t *power_cap); typedef struct adsb_level_report { uint64_t samples, negative, rail_lo, rail_hi, over; uint64_t hist[2048]; } adsb_level_report;
long adsb_level_device(adsb_decoder *d, const void *device_samples, size_t n, adsb_level_report *out, float *device_env, size_t env_cap); long adsb_level_device_as(adsb_decoder *d, int fmt, const void *device_samples, size_t n, adsb_level_report *out, float *device_env, size_t env_cap); long adsb_level_device_packed(adsb_decoder *d, const void *device_packed, size_t n, adsb_level_report *out, float *device_env, size_t env_cap); long adsb_level_device_iq(adsb_decoder *d, int fmt, const void *device_samples, size_t n, adsb_level_report *out, float *device_env, size_t env_cap); long adsb_level_device_power(adsb_decoder *d, const void *device_samples, size_t n, adsb_level_report *out, float *device_env, size_t env_cap); long adsb_level_host(adsb_decoder *d, const uint16_t *samples, size_t n, adsb_level_report *out, float *env, size_t env_cap); long adsb_level_batch_device(adsb_decoder *d, size_t n_captures, const void *const *device_samples, const size_t *n, adsb_level_report *out, float *const *device_env, const size_t *env_cap); long adsb_level_batch_device_as(adsb_decoder *d, int fmt, size_t n_captures, const void *const *device_samples, const size_t *n, adsb_level_report *out, float *const *device_env, const size_t *env_cap); long adsb_level_batch_device_packed(adsb_decoder *d, size_t n_captures, const void *const *device_packed, const size_t *n, adsb_level_report *out, float *const *device_env, const size_t *env_cap); long adsb_level_batch_device_iq(adsb_decoder *d, int fmt, size_t n_captures, const void *const *device_samples, const size_t *n, adsb_level_report *out, float *const *device_env, const size_t *env_cap); long adsb_level_batch_device_power(adsb_decoder *d, size_t n_captures, const void *const *device_samples, const size_t *n, adsb_level_report *out, float *const *device_env, const size_t *env_cap); long adsb_level_batch_host(adsb_decoder *d, size_t n_captures, const uint16_t *const *samples, const size_t *n, adsb_level_report *out, float *const *env, const size_t *env_cap); long adsb_level_windows(adsb_decoder *d, const void *device_samples, uint64_t first_sample, size_t n, size_t n_windows, const uint64_t *edges, adsb_level_report *out, float *device_env, size_t env_cap); long adsb_level_windows_host(adsb_decoder *d, const uint16_t *samples, uint64_t first_sample, size_t n, size_t n_windows, const uint64_t *edges, adsb_level_report *out, float *env, size_t env_cap); void adsb_level_add(adsb_level_report *sum, const adsb_level_report *part); float adsb_level_percentile(const adsb_level_report *r, double q); typedef struct adsb_burst { uint32_t begin, end, hot; float peak; } adsb_burst; /* runs of 28 power samples, [begin, end) */ long adsb_bursts_device(adsb_decoder *d, const float *device_env, size_t n_env, float threshold, uint32_t lead, uint32_t hang, adsb_burst *bursts, size_t cap); long adsb_bursts_host(adsb_decoder *d, const float *env, size_t n_env, float threshold, uint32_t lead, uint32_t hang, adsb_burst *bursts, size_t cap); typedef struct adsb_burst_carry { uint64_t runs; uint32_t open, first, last, hot; float peak; uint32_t reserved; } adsb_burst_carry; long adsb_bursts_slice_device(adsb_decoder *d, const float *device_env, size_t n_env, float threshold, uint32_t lead, uint32_t hang, const adsb_burst_carry *in, int final, adsb_burst *bursts, size_t cap, adsb_burst_carry *out); long adsb_bursts_slice_host(adsb_decoder *d, const float *env, size_t n_env, float threshold, uint32_t lead, uint32_t hang, const adsb_burst_carry *in, int final, adsb_burst *bursts, size_t cap, adsb_burst_carry *out); /* adsb_gather_*: KEEP ONLY THE BURSTS -- a capture of m power samples at sample_bytes bytes each (2: int8 IQ; 4: uint16 real, int16 IQ, float32 power; 8: float32 IQ) and an ordered burst table, as adsb_bursts_* returns it; piece i is the power samples [28 begin_i, min(28 end_i, m)), its bytes are capture[s lo_i : s hi_i]; the pieces lie in the output in table order, each from a multiple of 16 bytes on: offsets[0] = 0, offsets[i + 1] = round_up(offsets[i] + s (hi_i - lo_i), 16); pad bytes are zero; the total is offsets[n_bursts].  A piece's start is then a legal adsb_decode_batch_device* pointer (16-byte aligned, at a multiple of 4 samples), and on a flush handle (adsb_set_flush) the piece decodes as its silent twin: report g + 28 begin_i, which is exact, and ts + 28 begin_i, which is the original stream's ts only up to what accepted frames before the piece jumped (demod.c:99,128,134).  adsb_gather_layout: no device; offsets (n_bursts + 1, or NULL) and *total_bytes (or NULL) in host memory; 0, or -1 with adsb_last_error(NULL) naming the record: sample_bytes not 2, 4 or 8, a record with end <= begin or 28 begin >= m, records that do not ascend with a run between neighbours.  adsb_gather_device: device_capture and device_out in device memory, 16-byte aligned; bursts and offsets (n_bursts + 1, or NULL) in host memory; ONE launch on the handle's stream, returned when the bytes are there; returns the total bytes written (n_bursts 0: 0, nothing launched), nothing at or behind device_out + total is written; export rule 5 holds (callable between pushes).  Refused (-1, the message names the burst, nothing launched or written): what the layout refuses, capture_bytes < sample_bytes m, a pointer off 16 bytes or NULL with work to do, out_cap_bytes < total.  _as and _packed captures go through adsb_gather_pack12_* (their pieces are not in the capture's own bytes); no batch form, no joining across the slices of a stream, no multi-GPU form.  adsb_gather_pack12_*: THE SAME FOR A REAL CAPTURE AT 12 BITS -- n uint16 samples x carrying 12-bit codes, m = 2 (n / 4); piece i is the samples x[2 lo_i : 2 hi_i] completed to whole groups of 8 with code 2048 (at most four codes, only where m clips the last piece and m % 4 == 2), taken & 0x0fff and packed as Airspy packed 12-bit samples (ADSB_PACKED12_BYTES): 12 ceil((hi_i - lo_i) / 4) bytes, 84 per run, 3 per power sample where adsb_gather_device writes 4; offsets[i + 1] = round_up(offsets[i] + those, 16), pad bytes zero.  A piece's start is a legal adsb_decode_batch_device_packed pointer with n = 8 ceil((hi_i - lo_i) / 4), and on a flush handle it decodes as the uint16 piece does (the fill is the silence of its twin).  *over (or NULL): the pieces' OWN samples above 4095 -- never the fill, never a sample outside the pieces; their low 12 bits are what is stored.  _layout: no device, the table checked as adsb_gather_layout checks it.  _device: device_samples and device_out 16-byte aligned.  _as (fmt 1 | 3) / _packed (n % 8 == 0, 4-byte aligned): converted or unpacked first, by the launch and into the scratch of adsb_decode_device_as / _packed, then gathered from there; _as adds to adsb_get_format_report.  ONE gather launch on the handle's stream; returns the total bytes (n_bursts 0: 0, nothing launched), nothing at or behind device_out + total is written; export rules 5 and 6 hold.  Refused (-1, the message names the burst, nothing launched, written or counted): what the layout refuses, n >= 2^32, a capture or output pointer off 16 bytes (_packed's capture: 4) or NULL with work to do, out_cap_bytes < total, fmt not 1 or 3, _packed with n % 8 != 0.  Not built: gathering straight from a packed source without the unpack, IQ and power kinds, a batch form, stream slices, a multi-GPU form. */ long adsb_gather_layout(uint64_t m, int sample_bytes, const adsb_burst *bursts, size_t n_bursts, uint64_t *offsets, uint64_t *total_bytes); long adsb_gather_device(adsb_decoder *d, const void *device_capture, size_t capture_bytes, int sample_bytes, uint64_t m, const adsb_burst *bursts, size_t n_bursts, void *device_out, size_t out_cap_bytes, uint64_t *offsets); long adsb_gather_pack12_layout(uint64_t m, const adsb_burst *bursts, size_t n_bursts, uint64_t *offsets, uint64_t *total_bytes); long adsb_gather_pack12_device(adsb_decoder *d, const void *device_samples, size_t n, const adsb_burst *bursts, size_t n_bursts, void *device_out, size_t out_cap_bytes, uint64_t *offsets, uint64_t *over); long adsb_gather_pack12_device_as(adsb_decoder *d, int fmt, const void *device_samples, size_t n, const adsb_burst *bursts, size_t n_bursts, void *device_out, size_t out_cap_bytes, uint64_t *offsets, uint64_t *over); long adsb_gather_pack12_device_packed(adsb_decoder *d, const void *device_packed, size_t n, const adsb_burst *bursts, size_t n_bursts, void *device_out, size_t out_cap_bytes, uint64_t *offsets, uint64_t *over);
/* on = 1: no push refuses for length; the handle follows the reference's uint32_t sample counter (air.c:34) through its wraps, bit for bit.  Only on a
 * fresh or reset handle before the first push (else -1); sticky across adsb_reset.  adsb_get_wraps: wraps so far, and offsets of the seam kernel. adsb_set_flush (off by default; same rule: fresh or reset handle, sticky): decode a capture to its LAST sample instead of keeping the reference's end-of-file horizon (air.c:94-99, demod.c:89: the last ~41 k power samples are never scanned, a capture below 81 960 samples decodes nothing).  adsb_decode_device*, adsb_decode_batch_* and a stream ended by adsb_finish / a _final push then return, record for record and with the same Try/Ok table, what the reference returns for the capture's SILENT TWIN: its whole units (4 floor(n / 4) real samples, 2 floor(n / 2) IQ or power samples) followed by 81 960 power samples of silence (code 2048, (0, 0), +0.0) -- without padding or copying anything (DESIGN.md "Flush").  Every frame the horizon keeps comes back unchanged, in front.  Refuses, and is refused by, adsb_set_long_stream. */
int adsb_set_long_stream(adsb_decoder *d, int on); int adsb_get_wraps(const adsb_decoder *d, uint64_t *wraps, uint64_t *seam_offsets); int adsb_set_flush(adsb_decoder *d, int on); int adsb_get_flush(const adsb_decoder *d);
int adsb_finish(adsb_decoder *d); /* end of input (EOF, air.c:241-244): the remaining offsets and the end-of-file horizon (SURVEY Q10) */
/* Page-locked host buffers: the counterpart of `iqbuff = malloc(...)` (air.c:230), so that a push is one DMA.  adsb_host_alloc_on binds the memory to the NUMA node of `device` (best effort).  adsb_host_register page-locks memory the caller already owns.  0 / -1. */
void *adsb_host_alloc(size_t bytes); void *adsb_host_alloc_on(size_t bytes, int device); void adsb_host_free(void *p); int adsb_host_register(void *p, size_t bytes); int adsb_host_unregister(void *p);
/* Frame egress: what the reference hands to netout() (output.c:159), in its order.  adsb_drain copies (returns the number, <= cap, or -1);
 * adsb_take hands every pending frame out in place -- valid until the next call that pushes into, finishes, resets or destroys the handle. */
long adsb_drain(adsb_decoder *d, adsb_frame *out, size_t cap); long adsb_take(adsb_decoder *d, const adsb_frame **frames); size_t adsb_pending(const adsb_decoder *d);
/* print_stats() counters (valid.c:84-100); try_ needs collect_stats=1 (counted on the device, fetched by this call). */
int adsb_get_stats(const adsb_decoder *d, adsb_stats *out);
int adsb_get_profile_sized(const adsb_decoder *d, adsb_profile *out, size_t size); /* fills the first `size` bytes of *out: the macro passes the caller's sizeof */
#define adsb_get_profile(d, out) adsb_get_profile_sized((d), (out), sizeof(adsb_profile))
const char *adsb_last_error(const adsb_decoder *d); /* last error text of a handle, or of the last failed adsb_create() when d == NULL */
/* formatpkt() (output.c:204-262, WITH_AIR).  outformat 0 = AVR "*hex;\n", 1 = AVR-MLAT "@ts48hex;\n", 2 = Beast; pkt holds 256 bytes.  The length. */
int adsb_format_frame(const adsb_frame *f, int outformat, char *pkt);
/* The CPUs local to HIP device `device` (local_cpulist, e.g. "0-63,128-191") and its NUMA node (INTEGRATION.md, Deployment note).  The string's length, 0 if unknown, -1 / node or -1. */
int adsb_device_cpulist(int device, char *out, size_t cap); int adsb_device_numa_node(int device);
/* Splits the offsets [0, power_samples - ADSB_WINDOW] of one stream over n_shards owners (SURVEY.md 8e).  Shard i owns [g_begin[i], g_end[i])
 * (g_begin % 28 == 0) and needs the samples [first_sample[i], + n_samples[i]): 2 408 of halo.  Returns the shards used (<= n_shards). */
int adsb_plan_shards(uint64_t total_samples, int n_shards, uint64_t *g_begin, uint64_t *g_end, uint64_t *first_sample, uint64_t *n_samples);
/* ---- ONE process, several GPUs (csrc/multi.cpp; INTEGRATION.md "One process, several GPUs"): a worker thread and a decoder handle per device. */
typedef struct adsb_multi adsb_multi;
typedef struct adsb_multi_info { /* of the last adsb_multi_decode_* call */
    int32_t shards;         /* shards the capture was cut into (streams decoded side by side, for the stream calls)  */
    int32_t fallback;       /* 1: a seam was undecidable from the head candidates: ONE device decoded the capture as a stream (same frames) */
    uint64_t calls_walked;  /* deqframe calls the end-of-file walk replayed on the calling thread ...                */
    uint64_t calls_jumped;  /* ... and skipped by jumping onto the shards' own walks                                 */
    double create_ms;       /* adsb_multi_create: the slowest worker's adsb_create (the devices start side by side)  */
    double workers_ms;      /* the slowest worker's share of the call                                                */
    double stitch_us;       /* the stitcher on the calling thread                                                    */
    double serial_us;       /* everything behind the last worker: stitch + gather into one array                     */
    double total_ms;
    int32_t workers_bound;  /* workers whose thread runs on the CPUs of its device's NUMA node                       */
    int32_t helper_threads; /* sum of the workers' adsb_profile.host_threads_running after the call (each: adsb_multi_worker_profile)  */
} adsb_multi_info;
/* n_devices workers; devices[i] = HIP ordinal of worker i (NULL: 0 .. n_devices-1; an ordinal may repeat: plumbing tests
 * on a one-GPU box).  cfg as for adsb_create (device and stream are ignored).  NULL on failure (adsb_multi_last_error(NULL)). */
adsb_multi *adsb_multi_create(const adsb_config *cfg, int n_devices, const int *devices);
void adsb_multi_destroy(adsb_multi *m); int adsb_multi_devices(const adsb_multi *m);
/* ONE capture, time-sharded over as many devices as it is worth.  Returns the number of frames, in the reference's order, *frames valid until the
 * next call on m; -1 on failure (after a worker was given up the handle only answers -1, and that call's SOURCE buffers must stay alive).  _host: host
 * memory (page-lock it); _file: every worker reads its slice of a regular file; _device: slice i in worker i's HBM holds what adsb_multi_plan says. */
long adsb_multi_decode_host(adsb_multi *m, const uint16_t *samples, size_t n, const adsb_frame **frames); long adsb_multi_decode_file(adsb_multi *m, const char *path, const adsb_frame **frames);
long adsb_multi_decode_device(adsb_multi *m, uint64_t total_samples, const void *const *slices, int n_slices, const adsb_frame **frames);
int adsb_multi_plan(const adsb_multi *m, uint64_t total_samples, uint64_t *g_begin, uint64_t *g_end, uint64_t *first_sample, uint64_t *n_samples);
int adsb_multi_get_stats(const adsb_multi *m, adsb_stats *out); /* the stream's Try/Ok table (cfg.collect_stats) */
/* configs[3]: n_streams INDEPENDENT captures, stream s on worker s mod adsb_multi_devices(m), each with its own ts and
 * statistics -- N times what `adsbdec -f` does (main.c:60-89), side by side.  0 / -1; results per stream afterwards. */
int adsb_multi_set_long_streams(adsb_multi *m, int on); /* adsb_set_long_stream for the workers of the two stream calls below */
int adsb_multi_decode_streams_host(adsb_multi *m, int n_streams, const uint16_t *const *samples, const size_t *n); int adsb_multi_decode_streams_file(adsb_multi *m, int n_streams, const char *const *paths);
long adsb_multi_stream_frames(const adsb_multi *m, int stream, const adsb_frame **frames); int adsb_multi_stream_stats(const adsb_multi *m, int stream, adsb_stats *out);
int adsb_multi_get_info(const adsb_multi *m, adsb_multi_info *out);
/* n_captures INDEPENDENT captures over the devices, a contiguous range per worker in sub-batches (INTEGRATION.md).  packed != 0: Airspy packed 12-bit.
 * Results as adsb_decode_batch_host's, in capture order, valid until the next call on m; adsb_multi_get_stats: the sum.  _files: capture i is the regular
 * file paths[i] (uint16: size / 2 samples; packed: its whole 12-byte groups).  -1, no partial result: a worker failed or a file is unreadable. */
long adsb_multi_decode_batch_host(adsb_multi *m, size_t n_captures, const void *const *samples, const size_t *n, int packed,
                                  const adsb_frame **frames, uint64_t *first, adsb_stats *stats);
long adsb_multi_decode_batch_files(adsb_multi *m, size_t n_captures, const char *const *paths, int packed,
                                   const adsb_frame **frames, uint64_t *first, adsb_stats *stats);
/* A page-locked array for ONE capture that adsb_multi_decode_host will decode, every shard's part on the NUMA node of the
 * device that pulls it (free with adsb_host_free); adsb_multi_worker_placement says whether that held for the last decode. */
uint16_t *adsb_multi_host_alloc(adsb_multi *m, uint64_t total_samples);
typedef struct adsb_worker_placement {
    int32_t device, device_node; /* the worker's HIP device and its NUMA node (-1: the platform does not say)      */
    int32_t thread_bound;        /* the worker's thread runs on the CPUs of that node                              */
    int32_t slice_node;          /* the node most pages of the worker's slice of the last host capture live on     */
    double local_fraction;       /* share of the sampled pages of that slice on device_node (1.0 = fed from its socket) */
} adsb_worker_placement;
int adsb_multi_worker_placement(const adsb_multi *m, int worker, adsb_worker_placement *out);
/* adsb_get_profile of worker `worker`'s handle (first `size` bytes; the macro passes the caller's sizeof). */
int adsb_multi_worker_profile_sized(const adsb_multi *m, int worker, adsb_profile *out, size_t size);
#define adsb_multi_worker_profile(m, worker, out) adsb_multi_worker_profile_sized((m), (worker), (out), sizeof(adsb_profile))
const char *adsb_multi_last_error(const adsb_multi *m); /* of m; m == NULL: of the last failed adsb_multi_create(); names device and worker */
int adsb_abi_version(void);
#ifdef __cplusplus
}
#endif
#endif
