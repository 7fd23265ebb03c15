// batch.hpp -- a batch of INDEPENDENT captures in as few scan launches as they fit (adsb_decode_batch_*): where every capture
// lies in a launch, and how a launch's records become every capture's frames.  Host-only code, no HIP in it: it is part of
// the library through decoder_batch.hip and is tested without a device through adsb_batch_layout / adsb_batch_resolve
// (include/adsbdec_amd_diag.h).
//
// Layout: virtual stream coordinates.  The captures of a batch are laid end to end in ONE space of power-sample indices, capture
// i from the virtual offset V_i on, and a launch covers a stretch of that space: its records and try words carry g_rel = virtual
// offset - the launch's first one, 30 bits like those of any launch.  V_i is a multiple of 28: the FIR's ring phase (period 7
// pairs), the fs/4 sign (period 2) and the run boundaries (28) depend on the pair index only, so a capture whose pair 0 is
// called V_i sees exactly the arithmetic of a stream that starts at 0 (checked on the CPU against the oracle: silence of 14, 28,
// 56, 56 000 pairs in front of a capture leaves every power sample bit-identical; 8 does not).  The pairs below V_i read as
// silence (ScanArgs::p_lo), like those below 0 of a stream.  Behind a capture's last power sample at least one window plus one
// jump (kBatchGap) stay free, so that no offset of the next capture lies where a frame of this one could still reach.
// Tiles never straddle two captures: capture i's offsets take ceil(offsets / tile) tiles of their own, the last one partly
// filled -- the price of ONE K (passes per tile) per launch, which choose_batch_passes() keeps small.
// A capture whose offsets do not fit what is left of a launch (kBatchMaxLaunchOffsets) starts the next one; one that does not
// fit a launch at all is cut into SEGMENTS of whole tiles, a launch each.  Both decisions read ONE limit, which a test may lower
// (adsb_debug_config.batch_launch_offsets, batch_launch_limit) so that cut captures and roll-overs go through the kernel at
// sizes a test can afford.
//
// Resolve: a launch is collected after completion (sorted loose list + try list, as the stateless shard scan's), split at the
// virtual bases, and every capture goes through adsb::Resolver on its own -- reset, its candidates and tries rebased to offsets
// from 0, advance to ITS end of file -- so ts, the greedy skip, the end-of-file horizon and the Try/Ok table are the code that
// already has parity with the reference.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/adsbdec_amd_diag.h"
#include "resolver.hpp"

namespace adsb {

// the tile geometry of scan_kernel.h, which needs HIP to be read (decoder_batch.hip asserts that the two agree)
constexpr uint64_t kBatchRun = 28;
constexpr uint64_t batch_tile_offsets(int k) { return kBatchRun * (uint64_t)(252 * k - 44); }
constexpr uint64_t kBatchMaxLaunchOffsets = (1ull << 30) - batch_tile_offsets(32);
constexpr int kBatchSplitPasses = 7; // K of a launch that holds a piece of a capture too long for one launch
constexpr uint64_t kBatchGap = ADSB_WINDOW + ADSB_DECOFFSET; // 2 396: free virtual offsets behind a capture's last power sample

inline uint64_t batch_round_up(uint64_t v, uint64_t q) { return (v + q - 1) / q * q; }

// What the reference does with a file of n samples (air.c:59-99): power samples it produces by end of file (a trailing partial
// quad still yields two), and the offsets worth scanning -- none when its first deqframe call never fires (air.c:94: fewer than
// ADSB_APBUFFSZ power samples, i.e. 81 960 samples) or when no whole window exists.
inline uint64_t batch_power(uint64_t n) { return 2 * ((n + 3) / 4); }
inline uint64_t batch_offsets(uint64_t n)
{
    const uint64_t m = 2 * (n / 4);
    return (batch_power(n) >= ADSB_APBUFFSZ && m >= ADSB_WINDOW) ? m - ADSB_WINDOW + 1 : 0;
}
// The same for a flush handle (adsb_set_flush; resolver.hpp stream_end): the capture counts as its silent twin, whose power samples are
// those of its whole quads -- a trailing partial quad belongs to nothing -- and every one of them is an offset worth scanning: the
// windows that cross the capture's end read silence there (ScanArgs::p_hi), and the twin's offsets behind it hold nothing.
inline uint64_t batch_power_flush(uint64_t n) { return 2 * (n / 4); }
inline uint64_t batch_offsets_flush(uint64_t n) { return batch_power_flush(n); }

// One K for the segments [a, b): the K of 2 .. k_cap that computes the fewest runs -- a tile of K passes computes 252 K runs
// whatever part of it is owned or filled, so this weighs the halo (44 runs per tile: small K loses) against the partly filled
// last tile of every capture (half a tile on average: large K loses when captures are short).  k_cap is what an ordinary launch
// of as many offsets would take (scan_kernel.hip choose_passes: measured; beyond it larger tiles lose to the fill of the device).
inline int choose_batch_passes(const adsb_batch_segment *segs, size_t a, size_t b, int k_cap)
{
    int best = 2;
    uint64_t best_cost = ~0ull;
    for (int k = 2; k <= std::max(2, k_cap); k++) {
        uint64_t cost = 0;
        for (size_t i = a; i < b; i++)
            cost += (segs[i].o_end - segs[i].o_begin + batch_tile_offsets(k) - 1) / batch_tile_offsets(k) * (uint64_t)k;
        if (cost <= best_cost) {
            best = k;
            best_cost = cost;
        }
    }
    return best;
}

// The most virtual offsets a launch may cover: `wanted` (adsb_debug_config.batch_launch_offsets) where it holds a tile of a split
// launch at least and stays within what g_rel can say, else the default.
inline uint64_t batch_launch_limit(uint64_t wanted, int split_k)
{
    return (wanted >= batch_tile_offsets(split_k) && wanted <= kBatchMaxLaunchOffsets) ? wanted : kBatchMaxLaunchOffsets;
}

// Lay n_captures captures of n[i] samples out.  passes_cap(offsets, ctx): the K an ordinary launch of so many offsets takes;
// forced_passes > 0: that K for every launch (adsb_debug_config.passes); launch_offsets: batch_launch_limit's `wanted`.  Every
// capture has at least one segment (an empty one when it has no offsets), in capture order; a launch's segments are consecutive.
// false: a capture has 2^32 samples or more (*bad = its index) -- a batch has no long-stream mode.
inline bool batch_layout(size_t n_captures, const size_t *n, int (*passes_cap)(uint64_t, void *), void *ctx, int forced_passes,
                         uint64_t launch_offsets, std::vector<adsb_batch_segment> &segs, std::vector<adsb_batch_launch> &launches, size_t *bad,
                         bool flush = false)
{
    segs.clear();
    launches.clear();
    for (size_t i = 0; i < n_captures; i++)
        if ((uint64_t)n[i] >= (1ull << 32)) {
            if (bad)
                *bad = i;
            return false;
        }
    uint64_t V = 0; // next free virtual offset, a multiple of 28
    adsb_batch_launch cur{};
    auto close = [&](int split_passes) {
        cur.seg_end = (uint32_t)segs.size();
        if (cur.seg_end == cur.seg_first)
            return;
        uint64_t offsets = 0;
        for (size_t s = cur.seg_first; s < cur.seg_end; s++)
            offsets += segs[s].o_end - segs[s].o_begin;
        cur.passes = forced_passes > 0 ? forced_passes
                     : split_passes    ? split_passes
                                       : choose_batch_passes(segs.data(), cur.seg_first, cur.seg_end, passes_cap(offsets, ctx));
        cur.tiles = 0;
        cur.g_end = cur.g_begin;
        for (size_t s = cur.seg_first; s < cur.seg_end; s++) {
            adsb_batch_segment &sg = segs[s];
            sg.launch = (uint32_t)launches.size();
            sg.first_tile = cur.tiles;
            sg.tiles = (uint32_t)((sg.o_end - sg.o_begin + batch_tile_offsets(cur.passes) - 1) / batch_tile_offsets(cur.passes));
            cur.tiles += sg.tiles;
            if (sg.o_end > sg.o_begin)
                cur.g_end = sg.base + (sg.o_end - sg.o_begin);
        }
        launches.push_back(cur);
        cur = adsb_batch_launch{};
        cur.seg_first = (uint32_t)segs.size();
        cur.g_begin = V;
    };
    const int split_k = forced_passes > 0 ? forced_passes : kBatchSplitPasses;
    const uint64_t limit = batch_launch_limit(launch_offsets, split_k);
    const uint64_t split_piece = limit / batch_tile_offsets(split_k) * batch_tile_offsets(split_k);
    for (size_t i = 0; i < n_captures; i++) {
        const uint64_t n_off = flush ? batch_offsets_flush(n[i]) : batch_offsets(n[i]), power = flush ? batch_power_flush(n[i]) : batch_power(n[i]);
        uint64_t o = 0;
        for (;;) {
            const uint64_t rest = n_off - o;
            if (segs.size() == cur.seg_first)
                cur.g_begin = V; // a launch's g_rel counts from its first segment
            else if (rest > limit - std::min(limit, V - cur.g_begin))
                close(0); // does not fit what is left of this launch: the next one (which starts at V)
            adsb_batch_segment sg{};
            sg.capture = i;
            sg.o_begin = o;
            sg.base = V;
            const bool piece = rest > limit; // too long for any launch: whole tiles of it, a launch of their own
            sg.o_end = piece ? o + split_piece : n_off;
            segs.push_back(sg);
            // what the segment's offsets read: up to a window beyond the last one; a capture's last segment, up to its last power sample
            // (flush: the last segment's offsets end AT the last power sample, so the first term reaches ADSB_WINDOW - 1 offsets beyond
            // it -- silence by p_hi, whatever lies there -- and kBatchGap is counted from that reach, as it is from any other)
            const uint64_t reach = std::max(sg.o_end - sg.o_begin + (sg.o_end > sg.o_begin ? ADSB_WINDOW - 1 : 0), piece ? 0 : power - o);
            V = batch_round_up(V + reach + kBatchGap, kBatchRun);
            o = sg.o_end;
            if (!piece)
                break;
            close(split_k);
        }
    }
    close(0);
    return true;
}

// Sorted candidates and tries of a batch in virtual coordinates (cands[].g; tries (g << 2) | code) -> every capture's frames,
// one behind the other in `out` (capture i: out[first[i] .. first[i+1])), and its Try/Ok table (stats: null, or n_captures
// tables).  r: a resolver of the caller's, reset here for every capture.  cbuf / tbuf: scratch.  false: a record lies in no
// segment's offsets, or out of order.
inline bool batch_resolve(Resolver &r, size_t n_captures, const size_t *n, const adsb_batch_segment *segs, size_t n_segs,
                          const adsb_candidate *cands, size_t nc, const uint64_t *tries, size_t nt, std::vector<adsb_frame> &out,
                          uint64_t *first, adsb_stats *stats, std::vector<adsb_candidate> &cbuf, std::vector<uint64_t> &tbuf, bool flush = false)
{
    out.clear();
    size_t ci = 0, ti = 0, s = 0;
    for (size_t i = 0; i < n_captures; i++) {
        cbuf.clear();
        tbuf.clear();
        if (s >= n_segs || segs[s].capture != i)
            return false;
        for (; s < n_segs && segs[s].capture == i; s++) {
            const adsb_batch_segment &sg = segs[s];
            const uint64_t lo = sg.base, hi = sg.base + (sg.o_end - sg.o_begin);
            if ((ci < nc && cands[ci].g < lo) || (ti < nt && (tries[ti] >> 2) < lo))
                return false;
            for (; ci < nc && cands[ci].g < hi; ci++) {
                cbuf.push_back(cands[ci]);
                cbuf.back().g = cands[ci].g - lo + sg.o_begin;
            }
            for (; ti < nt && (tries[ti] >> 2) < hi; ti++)
                tbuf.push_back((((tries[ti] >> 2) - lo + sg.o_begin) << 2) | (tries[ti] & 3u));
        }
        first[i] = out.size();
        r.reset();
        if (!cbuf.empty() || !tbuf.empty()) { // (a capture without a record has no frame and no visited try)
            r.feed(cbuf.data(), cbuf.size(), tbuf.data(), tbuf.size());
            const StreamEnd e = stream_end(flush, batch_power_flush(n[i]), batch_power(n[i]), batch_offsets(n[i]));
            r.advance(e.power_samples, e.g_complete); // end of file: every offset has been fed (decoder.hip process_stage)
            const adsb_frame *fp = nullptr;
            const size_t nf = r.take(&fp);
            out.insert(out.end(), fp, fp + nf);
        }
        if (stats)
            stats[i] = r.stats();
    }
    first[n_captures] = out.size();
    r.reset();
    return ci == nc && ti == nt;
}

} // namespace adsb
