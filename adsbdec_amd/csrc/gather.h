// gather.h -- a capture's bursts as one array (include/adsbdec_amd.h: adsb_gather_*; gather_kernel.hip, decoder_gather.hip,
// host_abi.cpp).  The layout is adsbdec_amd/burst_archive.py layout: piece i is the power samples [28 begin_i, min(28 end_i, M)) of
// a capture of M power samples at s bytes each, its bytes are capture[s lo_i : s hi_i], the pieces lie in table order, each from a
// multiple of 16 bytes on, and the pad bytes are zero.  Host code (the one HIP declaration is behind __HIPCC__): host_abi.cpp is
// built without HIP and sizes an output with gather_layout alone.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/adsbdec_amd.h"

#pragma GCC visibility push(hidden)

namespace adsb {

constexpr uint64_t kGatherRun = 28;     // power samples per run: a burst's unit (level.h)
constexpr unsigned kGatherChunk = 256;  // C: consecutive 16-byte output words a block looks its rows up for at once (= its lanes)

// A row per piece, in table order: its output words are w_first .. (the next row's w_first - 1), word k of them is the bytes
// [src + 16 k, min(src + 16 k + 16, src + bytes)) of the capture, zero-padded.  Row B, behind the last one, holds the number of
// all words.  Every piece has a byte, so w_first ascends strictly.
struct GatherRow {
    uint64_t w_first;
    uint64_t src;   // byte offset into the capture: s 28 begin, a multiple of 8
    uint64_t bytes; // s (hi - lo)
};

// The layout and its refusals.  offsets: NULL, or n_bursts + 1 byte offsets; rows: NULL, or n_bursts + 1 rows.  Returns 0, or -1
// with the reason in why[why_cap], which names the record.
inline int gather_layout(uint64_t m, int sample_bytes, const adsb_burst *bursts, size_t n_bursts, uint64_t *offsets, GatherRow *rows,
                         uint64_t *total_bytes, char *why, size_t why_cap)
{
    if (sample_bytes != 2 && sample_bytes != 4 && sample_bytes != 8) {
        snprintf(why, why_cap, "sample_bytes = %d is none of 2 (int8 IQ), 4 (uint16 real, int16 IQ, float32 power), 8 (float32 IQ)", sample_bytes);
        return -1;
    }
    if (!bursts && n_bursts) {
        snprintf(why, why_cap, "NULL table with n_bursts = %zu", n_bursts);
        return -1;
    }
    if (m >= (1ull << 59)) { // (s m stays below 2^62)
        snprintf(why, why_cap, "m = %llu power samples is 2^59 or more", (unsigned long long)m);
        return -1;
    }
    const uint64_t s = (uint64_t)sample_bytes;
    uint64_t off = 0;
    for (size_t i = 0; i < n_bursts; i++) {
        const adsb_burst &b = bursts[i];
        if (b.end <= b.begin) {
            snprintf(why, why_cap, "burst %zu: end = %u is not above begin = %u", i, b.end, b.begin);
            return -1;
        }
        if (kGatherRun * b.begin >= m) {
            snprintf(why, why_cap, "burst %zu: begin = %u is run %u's power sample %llu, outside the capture's m = %llu", i, b.begin, b.begin,
                     (unsigned long long)(kGatherRun * b.begin), (unsigned long long)m);
            return -1;
        }
        if (i && b.begin <= bursts[i - 1].end) {
            snprintf(why, why_cap, "burst %zu: begin = %u does not leave a run behind burst %zu's end = %u (a table ascends, with a run between neighbours)",
                     i, b.begin, i - 1, bursts[i - 1].end);
            return -1;
        }
        const uint64_t lo = kGatherRun * b.begin, hi = kGatherRun * b.end < m ? kGatherRun * b.end : m;
        if (offsets)
            offsets[i] = off;
        if (rows)
            rows[i] = GatherRow{off / 16, s * lo, s * (hi - lo)};
        off = (off + s * (hi - lo) + 15) & ~(uint64_t)15;
    }
    if (offsets)
        offsets[n_bursts] = off;
    if (rows)
        rows[n_bursts] = GatherRow{off / 16, 0, 0};
    if (total_bytes)
        *total_bytes = off;
    return 0;
}

#ifdef __HIPCC__
// gather_kernel.hip: the `words` 16-byte words of n_rows pieces from `capture` to `out` (both 16-byte aligned), ONE launch on
// `stream`.
hipError_t launch_gather(void *out, const void *capture, const GatherRow *tab_device, uint32_t n_rows, uint64_t words, hipStream_t stream);
#endif

} // namespace adsb

#pragma GCC visibility pop
