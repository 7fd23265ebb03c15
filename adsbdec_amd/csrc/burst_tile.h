// burst_tile.h -- the gate's three kernels, stated once for the two units that launch them: burst_kernel.hip (adsb_bursts_*: one
// envelope, runs counted from its first float, records clipped to it) and burst_slice_kernel.hip (adsb_bursts_slice_*: a SLICE of
// a stream).  The unit says which before it includes this file: ADSB_BURST_SLICE 0 or 1.  The shape is described in
// burst_kernel.hip; the lines of that unit were moved here word for word, and with ADSB_BURST_SLICE 0 the compiler sees exactly
// them (profiles/r36_burst_slice_isa_identity.txt).  A slice differs in three places, each under #if:
//   runs      are STREAM runs: the slice's first float is run BurstSlice::first_run, and every index below is one of the stream
//   combine   starts from the carried cluster instead of from nothing: its last hot run is the hot run before tile 0 and it counts
//             as one start in front of the slice, so the carried cluster is burst 0 whether a hot run of the slice joins it or not
//   emit      clips begin at run 0 of the stream and end nowhere, and the LAST burst (k = B - 1, the one that may stay open) goes
//             to the slot behind the cap records, as {its first hot run, its last hot run + 1 (0: none in this slice), hot, peak}:
//             whatever the cap, the host has the true ends of the cluster it may have to carry on
#pragma once

#include "burst.h"

#ifndef ADSB_BURST_SLICE
#error "burst_tile.h: define ADSB_BURST_SLICE as 0 (a capture) or 1 (a slice of a stream) first"
#endif
#if ADSB_BURST_SLICE
#define ADSB_BURST_KERNEL(name) burst_slice_##name
#define ADSB_BURST_PARAMS const BurstArgs a, const BurstSlice sl
// where burst k's record lies and whether it has a place: the records below the cap, and the last burst behind them (cap <= B - 1)
#define ADSB_BURST_KEPT(k) ((k) < a.cap || (k) == last_k)
#define ADSB_BURST_SLOT(k) ((k) < a.cap ? (k) : a.cap)
#else
#define ADSB_BURST_KERNEL(name) burst_##name
#define ADSB_BURST_PARAMS const BurstArgs a
#define ADSB_BURST_KEPT(k) k < a.cap
#define ADSB_BURST_SLOT(k) k
#endif

namespace adsb {

namespace {

constexpr int kLanes = 256, kTileWaves = 4, kPerLane = 8;
static_assert((uint32_t)kLanes * kPerLane == kBurstTileRuns, "a lane holds eight runs of its tile");

__device__ __forceinline__ uint32_t sign_clear(uint32_t b) { return (b >> 31) ? 0u : b; }

// The lane's eight runs: grid indices v0 .. v0 + 7 (v0 a multiple of 8: both quads 16-byte aligned), run r = v - pad.
struct LaneRuns {
    uint32_t u[kPerLane];
    uint32_t hot;   // bit j: run j is inside the envelope and hot
    uint32_t r0;    // the run of slot 0 (wraps below zero where slot 0 lies in front of the envelope: never used there)
    __device__ uint32_t first() const { return r0 + (uint32_t)__builtin_ctz(hot); }
    __device__ uint32_t last() const { return r0 + 31u - (uint32_t)__builtin_clz(hot); }
};

__device__ __forceinline__ void load_runs(const BurstArgs &a, uint32_t tile, LaneRuns &x)
{
    const uint32_t v0 = tile * kBurstTileRuns + threadIdx.x * kPerLane;
    const uint32_t lo = a.pad, hi = a.pad + a.runs; // the envelope on the grid
    uint32_t valid = 0;
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const uint32_t v = v0 + 4 * q;
        if (v >= lo && v + 4 <= hi) {
            const uint4 w = *reinterpret_cast<const uint4 *>(a.base + v);
            x.u[4 * q] = sign_clear(w.x), x.u[4 * q + 1] = sign_clear(w.y), x.u[4 * q + 2] = sign_clear(w.z), x.u[4 * q + 3] = sign_clear(w.w);
            valid |= 0xFu << (4 * q);
        } else { // the head or the tail of an envelope: only the floats that are its own
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const bool in = v + j >= lo && v + j < hi;
                x.u[4 * q + j] = in ? sign_clear(__float_as_uint(a.base[v + j])) : 0u;
                valid |= (in ? 1u : 0u) << (4 * q + j);
            }
        }
    }
    x.hot = 0;
#pragma unroll
    for (int j = 0; j < kPerLane; j++)
        x.hot |= (x.u[j] >= a.threshold_bits ? 1u : 0u) << j;
    x.hot &= valid;
    x.r0 = v0 - a.pad;
}

// The lane's neighbours in its wave: the last hot run of the nearest lower lane that has one, the first of the nearest upper one
// (kBurstNone: none in the wave), and the wave's own first and last.
struct WaveView {
    uint32_t before, after, first, last;
};

__device__ __forceinline__ WaveView wave_view(const LaneRuns &x)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long any = __ballot(x.hot != 0);
    const uint32_t mine_first = x.hot ? x.first() : kBurstNone, mine_last = x.hot ? x.last() : kBurstNone;
    const unsigned long long below = any & ((1ull << lane) - 1), above = lane == 63 ? 0ull : any & (~0ull << (lane + 1));
    const uint32_t from_below = __shfl(mine_last, below ? 63 - __builtin_clzll(below) : 0);
    const uint32_t from_above = __shfl(mine_first, above ? __builtin_ctzll(above) : 0);
    const uint32_t w_first = __shfl(mine_first, any ? __builtin_ctzll(any) : 0);
    const uint32_t w_last = __shfl(mine_last, any ? 63 - __builtin_clzll(any) : 0);
    WaveView w;
    w.before = below ? from_below : kBurstNone;
    w.after = above ? from_above : kBurstNone;
    w.first = any ? w_first : kBurstNone;
    w.last = any ? w_last : kBurstNone;
    return w;
}

// ---- 1: the summaries ----
__global__ __launch_bounds__(kLanes) void ADSB_BURST_KERNEL(summary_kernel)(ADSB_BURST_PARAMS)
{
    __shared__ uint32_t w_first[kTileWaves], w_last[kTileWaves], w_starts[kTileWaves];
    const uint32_t tile = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    LaneRuns x;
    load_runs(a, tile, x);
#if ADSB_BURST_SLICE
    x.r0 += sl.first_run;
#endif
    const WaveView w = wave_view(x);
    // starts among the lane's hot runs, the wave's first hot run left out (whether it is one is the tile's or the combine's to say)
    uint32_t starts = 0, prev = w.before;
#pragma unroll
    for (int j = 0; j < kPerLane; j++)
        if (x.hot >> j & 1) {
            const uint32_t r = x.r0 + j;
            starts += prev != kBurstNone && r - prev > a.join;
            prev = r;
        }
#pragma unroll
    for (int off = 32; off; off >>= 1)
        starts += __shfl_xor(starts, off);
    if (lane == 0)
        w_first[wave] = w.first, w_last[wave] = w.last, w_starts[wave] = starts;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t first = kBurstNone, last = kBurstNone, inner = 0;
        for (int k = 0; k < kTileWaves; k++) {
            inner += w_starts[k];
            if (w_first[k] == kBurstNone)
                continue;
            if (last != kBurstNone && w_first[k] - last > a.join)
                inner++;
            if (first == kBurstNone)
                first = w_first[k];
            last = w_last[k];
        }
        *reinterpret_cast<uint4 *>(a.summaries + (size_t)tile * kBurstTileWords) = make_uint4(first, last, inner, 0u);
    }
}

// ---- 2: the combine ----
// An inclusive scan over the workgroup's 256 values in LDS, lane `pos` holding position pos; -> the value at pos - 1 combined with
// nothing (the exclusive result; `identity` at position 0) and, in *all, the combination of all 256.
template <class Op>
__device__ __forceinline__ uint32_t scan_exclusive(uint32_t *s, int pos, uint32_t x, uint32_t identity, Op op, uint32_t *all)
{
    __syncthreads(); // (whoever still reads s from the scan before)
    s[pos] = x;
    __syncthreads();
    for (int off = 1; off < kLanes; off <<= 1) {
        uint32_t y = s[pos];
        if (pos >= off)
            y = op(s[pos - off], y);
        __syncthreads();
        s[pos] = y;
        __syncthreads();
    }
    *all = s[kLanes - 1];
    return pos ? s[pos - 1] : identity;
}

__global__ __launch_bounds__(kLanes) void ADSB_BURST_KERNEL(combine_kernel)(ADSB_BURST_PARAMS)
{
    __shared__ uint32_t s[kLanes];
    const int t = threadIdx.x;
    const uint32_t chunks = (a.n_tiles + kLanes - 1) / kLanes;
    const auto umin = [](uint32_t p, uint32_t q) { return p < q ? p : q; };
    const auto umax = [](uint32_t p, uint32_t q) { return p > q ? p : q; };
    const auto uadd = [](uint32_t p, uint32_t q) { return p + q; };
    // backwards: the hot run after every tile = the smallest first hot run of the tiles behind it (kBurstNone is the largest value)
    uint32_t carry = kBurstNone;
    for (uint32_t c = chunks; c-- > 0;) {
        const uint32_t i = c * kLanes + t;
        const uint32_t first = i < a.n_tiles ? a.summaries[(size_t)i * kBurstTileWords] : kBurstNone;
        uint32_t all;
        const uint32_t behind = scan_exclusive(s, kLanes - 1 - t, first, kBurstNone, umin, &all);
        if (i < a.n_tiles)
            a.rows[(size_t)i * kBurstTileWords + 1] = umin(behind, carry);
        carry = umin(all, carry);
    }
    // forwards: the hot run before every tile (kept as run + 1, 0 = none: the largest wins), whether the tile's first hot run is a
    // start, and the starts before the tile
    uint32_t carry_last = 0, carry_starts = 0;
#if ADSB_BURST_SLICE
    carry_last = sl.prev_last1, carry_starts = sl.prev_starts;
#endif
    for (uint32_t c = 0; c < chunks; c++) {
        const uint32_t i = c * kLanes + t;
        uint4 sum = make_uint4(kBurstNone, kBurstNone, 0u, 0u);
        if (i < a.n_tiles)
            sum = *reinterpret_cast<const uint4 *>(a.summaries + (size_t)i * kBurstTileWords);
        const bool hot = sum.x != kBurstNone;
        uint32_t all_last, all_starts;
        const uint32_t before1 = umax(scan_exclusive(s, t, hot ? sum.y + 1 : 0u, 0u, umax, &all_last), carry_last);
        const uint32_t is_start = hot && (before1 == 0 || sum.x - (before1 - 1) > a.join);
        const uint32_t starts_before = scan_exclusive(s, t, hot ? sum.z + is_start : 0u, 0u, uadd, &all_starts) + carry_starts;
        if (i < a.n_tiles) {
            uint32_t *row = a.rows + (size_t)i * kBurstTileWords;
            row[0] = before1 ? before1 - 1 : kBurstNone;
            row[2] = is_start;
            row[3] = starts_before;
        }
        carry_last = umax(all_last, carry_last);
        carry_starts += all_starts;
    }
    if (t == 0)
        *a.total = carry_starts;
}

// ---- 3: the emit ----
__device__ __forceinline__ void add_to_burst(const BurstArgs &a, uint32_t k, uint32_t hot, uint32_t peak)
{
    atomicAdd(a.table + (size_t)k * 4 + 2, hot);
    atomicMax(a.table + (size_t)k * 4 + 3, peak);
}

__global__ __launch_bounds__(kLanes) void ADSB_BURST_KERNEL(emit_kernel)(ADSB_BURST_PARAMS)
{
    __shared__ uint32_t w_first[kTileWaves], w_last[kTileWaves], w_starts[kTileWaves];
    const uint32_t tile = blockIdx.x;
    const uint4 row = *reinterpret_cast<const uint4 *>(a.rows + (size_t)tile * kBurstTileWords);
    if (a.summaries[(size_t)tile * kBurstTileWords] == kBurstNone) // (the whole workgroup: nothing of this tile is hot)
        return;
#if ADSB_BURST_SLICE
    const uint32_t last_k = *a.total - 1; // (B >= 1: a tile has a hot run)
#endif
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    LaneRuns x;
    load_runs(a, tile, x);
#if ADSB_BURST_SLICE
    x.r0 += sl.first_run;
#endif
    const WaveView w = wave_view(x);
    if (lane == 0)
        w_first[wave] = w.first, w_last[wave] = w.last;
    __syncthreads();
    // the hot run before the lane's first and the one behind its last: in the wave, else in the tile's other waves, else the row's
    uint32_t before = w.before, after = w.after;
    if (before == kBurstNone) {
        before = row.x;
        for (int k = 0; k < wave; k++)
            if (w_last[k] != kBurstNone)
                before = w_last[k];
    }
    if (after == kBurstNone) {
        after = row.y;
        for (int k = kTileWaves - 1; k > wave; k--)
            if (w_first[k] != kBurstNone)
                after = w_first[k];
    }
    // the starts among the lane's hot runs, and with them the starts in front of the lane
    uint32_t starts = 0, prev = before;
#pragma unroll
    for (int j = 0; j < kPerLane; j++)
        if (x.hot >> j & 1) {
            const uint32_t r = x.r0 + j;
            starts += prev == kBurstNone || r - prev > a.join;
            prev = r;
        }
    uint32_t upto = starts; // inclusive over the wave's lanes
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t y = __shfl_up(upto, off);
        if (lane >= off)
            upto += y;
    }
    if (lane == 63)
        w_starts[wave] = upto;
    __syncthreads();
    uint32_t count = row.w + upto - starts; // starts in front of the lane's runs, in the whole envelope
    for (int k = 0; k < wave; k++)
        count += w_starts[k];
    // the lane's hot runs, one by one: burst k = (starts up to and including the run) - 1
    uint32_t seg_k = kBurstNone, seg_hot = 0, seg_peak = 0;
    prev = before;
#pragma unroll
    for (int j = 0; j < kPerLane; j++)
        if (x.hot >> j & 1) {
            const uint32_t r = x.r0 + j;
            const bool start = prev == kBurstNone || r - prev > a.join;
            prev = r;
            count += start;
            const uint32_t k = count - 1; // (count >= 1: a hot run that is no start has a start in front of it)
            const uint32_t rest = x.hot >> j >> 1;
            const uint32_t next = rest ? r + 1 + (uint32_t)__builtin_ctz(rest) : after;
            const bool end = next == kBurstNone || next - r > a.join;
            if (k != seg_k) {
                if (seg_hot && ADSB_BURST_KEPT(seg_k))
                    add_to_burst(a, ADSB_BURST_SLOT(seg_k), seg_hot, seg_peak);
                seg_k = k, seg_hot = 0, seg_peak = 0;
            }
            seg_hot++;
            seg_peak = x.u[j] > seg_peak ? x.u[j] : seg_peak;
#if ADSB_BURST_SLICE
            if (ADSB_BURST_KEPT(k)) {
                uint32_t *rec = a.table + (size_t)ADSB_BURST_SLOT(k) * 4;
                const bool raw = k == last_k;
                if (start)
                    rec[0] = raw ? r : r >= a.lead ? r - a.lead : 0u;
                if (end)
                    rec[1] = raw ? r + 1 : r + a.hang + 1;
            }
#else
            if (k < a.cap) {
                if (start)
                    a.table[(size_t)k * 4] = r >= a.lead ? r - a.lead : 0u;
                if (end)
                    a.table[(size_t)k * 4 + 1] = r + a.hang + 1 < a.runs ? r + a.hang + 1 : a.runs;
            }
#endif
        }
    // what the lane still holds: where every lane of the wave that holds something holds the same burst, one lane adds for all
    const bool have = seg_hot != 0 && ADSB_BURST_KEPT(seg_k);
    const unsigned long long holders = __ballot(have);
    if (holders == 0)
        return;
    const uint32_t k0 = __shfl(seg_k, __builtin_ctzll(holders));
    if (__ballot(have && seg_k == k0) == holders) {
        uint32_t hot = have ? seg_hot : 0u, peak = have ? seg_peak : 0u;
#pragma unroll
        for (int off = 32; off; off >>= 1) {
            hot += __shfl_xor(hot, off);
            const uint32_t y = __shfl_xor(peak, off);
            peak = y > peak ? y : peak;
        }
        if (lane == 0)
            add_to_burst(a, ADSB_BURST_SLOT(k0), hot, peak);
    } else if (have) {
        add_to_burst(a, ADSB_BURST_SLOT(seg_k), seg_hot, seg_peak);
    }
}

} // namespace

} // namespace adsb

#undef ADSB_BURST_KERNEL
#undef ADSB_BURST_PARAMS
#undef ADSB_BURST_KEPT
#undef ADSB_BURST_SLOT
