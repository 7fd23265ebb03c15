// gather_pack12.h -- a real capture's bursts as one array of Airspy packed 12-bit samples (include/adsbdec_amd.h: adsb_gather_pack12_*;
// gather_pack12_kernel.hip, decoder_gather_pack12.hip, host_abi.cpp).  The layout is adsbdec_amd/burst_archive.py layout12: the
// capture is n uint16 samples x carrying 12-bit codes, M = 2 (n / 4) power samples; piece i is the power samples
// [lo, hi) = [28 begin_i, min(28 end_i, M)), that is the samples x[2 lo : 2 hi], completed to whole groups of 8 with code 2048, taken
// & 0xfff and packed (packed12.h pack12_group): 12 ceil((hi - lo) / 4) bytes.  The pieces lie in table order, each from a multiple of
// 16 bytes on, and the pad bytes are zero.  Host code (the one HIP declaration is behind __HIPCC__), as gather.h is.
#pragma once

#include "gather.h"

#pragma GCC visibility push(hidden)

namespace adsb {

#ifndef ADSB_GATHER_PACK12_LANE3
#define ADSB_GATHER_PACK12_LANE3 0 // 1 (a measurement build): a lane turns four groups into three words -- see gather_pack12_kernel.hip
#endif

constexpr uint32_t kPack12Fill = 2048; // the code behind a clipped last piece's samples: the silence the decoders read outside a buffer

// A row per piece, in table order: its output words are w_first .. (the next row's w_first - 1); its groups are the samples
// [src + 8 j, src + 8 j + 8) of the capture, j < samples / 8, of which the first `own` samples exist (own = samples, or 4 less)
// and the rest are kPack12Fill.  Row B, behind the last one, holds the number of all words.
struct GatherPack12Row {
    uint64_t w_first;
    uint64_t src;     // sample offset into the capture: 56 begin, a multiple of 8
    uint64_t samples; // 8 ceil((hi - lo) / 4): what a batch decode call is told
    uint64_t own;     // 2 (hi - lo)
#if ADSB_GATHER_PACK12_LANE3
    uint64_t t_first; // the piece's first TRIPLE of words (four groups): what that build numbers instead of words
#endif
};

// The layout and its refusals: those of gather_layout at 4 bytes per power sample (a table is checked as it is there).  offsets:
// NULL, or n_bursts + 1 byte offsets; rows: NULL, or n_bursts + 1 rows.  Returns 0, or -1 with the reason in why[why_cap].
inline int gather_pack12_layout(uint64_t m, const adsb_burst *bursts, size_t n_bursts, uint64_t *offsets, GatherPack12Row *rows,
                                uint64_t *total_bytes, char *why, size_t why_cap)
{
    if (gather_layout(m, 4, bursts, n_bursts, nullptr, nullptr, nullptr, why, why_cap))
        return -1;
    uint64_t off = 0;
#if ADSB_GATHER_PACK12_LANE3
    uint64_t triples = 0;
#endif
    for (size_t i = 0; i < n_bursts; i++) {
        const adsb_burst &b = bursts[i];
        const uint64_t lo = kGatherRun * b.begin, hi = kGatherRun * b.end < m ? kGatherRun * b.end : m;
        const uint64_t groups = (hi - lo + 3) / 4;
        if (offsets)
            offsets[i] = off;
#if ADSB_GATHER_PACK12_LANE3
        if (rows)
            rows[i] = GatherPack12Row{off / 16, 2 * lo, 8 * groups, 2 * (hi - lo), triples};
        triples += (groups + 3) / 4;
#else
        if (rows)
            rows[i] = GatherPack12Row{off / 16, 2 * lo, 8 * groups, 2 * (hi - lo)};
#endif
        off = (off + 12 * groups + 15) & ~(uint64_t)15;
    }
    if (offsets)
        offsets[n_bursts] = off;
#if ADSB_GATHER_PACK12_LANE3
    if (rows)
        rows[n_bursts] = GatherPack12Row{off / 16, 0, 0, 0, triples};
#else
    if (rows)
        rows[n_bursts] = GatherPack12Row{off / 16, 0, 0, 0};
#endif
    if (total_bytes)
        *total_bytes = off;
    return 0;
}

#ifdef __HIPCC__
// gather_pack12_kernel.hip: the `words` 16-byte words of n_rows pieces from the uint16 `capture` to `out` (both 16-byte aligned),
// the pieces' own samples above 4095 added to *over (device memory, zeroed by the caller on `stream`), ONE launch on `stream`.
// (The measurement build ADSB_GATHER_PACK12_LANE3 takes the number of all TRIPLES, the closing row's t_first, for `words`.)
hipError_t launch_gather_pack12(void *out, const uint16_t *capture, const GatherPack12Row *tab_device, uint32_t n_rows, uint64_t words,
                                unsigned long long *over, hipStream_t stream);
#endif

} // namespace adsb

#pragma GCC visibility pop
