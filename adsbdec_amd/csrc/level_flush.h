// level_flush.h -- how a wave of level_batch_kernel.hip (a batch of captures) and of level_windows_kernel.hip (the windows of one
// stream) hands its counts over, device code shared by the two: the wave's histogram in LDS belongs to ONE row of the launch's
// table at a time -- a capture, a window -- and goes to that row's totals when the row changes and at the wave's end; the four
// waves of a workgroup leave as one sum where they end in the same row.  Moved here from level_batch_kernel.hip word for word
// when the windows unit came: everything is forced inline in an anonymous namespace, and level_batch_kernel.hip compiles to the
// instructions it had with these lines of its own (profiles/r27_level_windows_isa_identity.txt).
// Included behind scan_stages.h (kWaves, kThreads), level.h (kLevelBins, kLevelWords) and level_tail.h (Counts).
#pragma once

#ifndef ADSB_LEVEL_BATCH_MERGE
#define ADSB_LEVEL_BATCH_MERGE 1 // 0 in a measurement build: every wave flushes alone at its end (DESIGN.md section 4 "Batch level report")
#endif

namespace adsb {

namespace {

constexpr int kBinsPerLane = kLevelBins / 64;

// what the wave has written to its histogram is there for every lane of it to read, and the other way round
__device__ __forceinline__ void wave_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ void wave_begin(uint32_t *hist, const int lane)
{
#pragma unroll
    for (int j = 0; j < kBinsPerLane; j++)
        hist[64 * j + lane] = 0;
    wave_sync();
}

// the wave's counters go to the totals of the capture they belong to
__device__ __forceinline__ void counts_flush(Counts &c, unsigned long long *__restrict__ tot, const int lane)
{
    if (lane == 0) {
        if (c.negative)
            atomicAdd(&tot[1], (unsigned long long)c.negative);
        if (c.rail_lo)
            atomicAdd(&tot[2], (unsigned long long)c.rail_lo);
        if (c.rail_hi)
            atomicAdd(&tot[3], (unsigned long long)c.rail_hi);
        if (c.over)
            atomicAdd(&tot[4], (unsigned long long)c.over);
    }
    c = Counts{};
}

// The wave's counts go to the totals of the capture they belong to, and the wave holds nothing again.
__device__ __forceinline__ void wave_flush(uint32_t *hist, Counts &c, unsigned long long *__restrict__ tot, const int lane)
{
    wave_sync();
#pragma unroll 4
    for (int j = 0; j < kBinsPerLane; j++) {
        const int bin = 64 * j + lane;
        const uint32_t v = hist[bin];
        if (v) {
            atomicAdd(&tot[5 + bin], (unsigned long long)v);
            hist[bin] = 0;
        }
    }
    counts_flush(c, tot, lane);
    wave_sync();
}

// Behind a wave's last pass: what it still holds (held: of the capture whose totals are number `tot`) leaves.  The workgroup's four
// waves meet here; where all hold the same capture their histograms are summed first and leave in one add per bin.
__device__ __forceinline__ void block_finish(uint32_t (*hist)[kLevelBins], uint32_t *who, Counts &c, const bool held, const uint32_t tot,
                                             unsigned long long *__restrict__ totals, const int lane, const int wave_in_block)
{
#if ADSB_LEVEL_BATCH_MERGE
    if (lane == 0)
        who[wave_in_block] = held ? tot : 0xFFFFFFFFu; // (never a row: rows are indexed below 2^32 - 1)
    __syncthreads();
    const uint32_t t0 = who[0];
    bool same = t0 != 0xFFFFFFFFu; // (workgroup-uniform)
#pragma unroll
    for (int w = 1; w < kWaves; w++)
        same = same && who[w] == t0;
    if (same) {
        unsigned long long *tt = totals + (size_t)t0 * kLevelWords;
        counts_flush(c, tt, lane);
#pragma unroll
        for (int j = 0; j < kLevelBins / kThreads; j++) {
            const int bin = j * kThreads + threadIdx.x;
            uint32_t v = 0;
#pragma unroll
            for (int w = 0; w < kWaves; w++)
                v += hist[w][bin];
            if (v)
                atomicAdd(&tt[5 + bin], (unsigned long long)v);
        }
        return;
    }
#endif
    if (held)
        wave_flush(hist[wave_in_block], c, totals + (size_t)tot * kLevelWords, lane);
}

} // namespace

} // namespace adsb
