// scan_tile.h -- the shell of a scan tile, the same around every front end: the LDS carve-up, the planes' pad words, Stage A, a
// barrier, Stage B, the profile clocks; the start stagger; and, host side, the two launchers behind the kernels.  The scan
// units (scan_kernel.hip and the units of the other front ends) keep their __global__ entries -- the lines that find a
// tile's K, its samples and its first offset -- and hand the rest to scan_tile<kStats, kFront>.
//
// This header does NOT include scan_stages.h, whose stages it calls: a unit includes scan_stages.h first, then this.
// tools/position_sweep_mutants.py compiles copies of the units beside a mutated scan_stages.h and reaches every other header
// through -I; a quote-include from here, inside csrc/, would find the unmutated file a second time (#pragma once is per
// file), and the build would hold both.
//
// What is shared and what is not follows the compiled code (DESIGN.md "The tile shell"; profiles/r31_tile_shell_isa_identity.txt):
//  - Stage A is chosen by `if constexpr` inside scan_tile.  A forwarding function stage_a_of<kFront>(...) with __restrict__
//    parameters reordered two LDS stores and renamed registers in the IQ unit (42 lines of its gfx950 code).
//  - The entries' own lines (K, the stagger, prof_begin, a batch tile's segment, t0) stay in the kernels: moved into a shared
//    inlined body they moved about 250 lines of code per unit.  A helper for the batch entries' eight segment lines
//    (segs[tile_seg[blockIdx.x]] -> ScanArgs, with the address-space cast) was tried too: 127-129 lines per front-end unit.
//  - scan_batch_kernel.hip keeps the shell in its own lines (over scan_tile its <false> instantiation's scalar registers are
//    renamed inside Stage B's loops) and uses the stagger and the launcher from here, which leave its code as it was.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_kernel.h"
#include "scan_stamps.h" // ADSB_STAMP / ADSB_COUNT: nothing but in a measurement build of scan_kernel.hip (the other units #undef its switch)

namespace adsb {

// The kMinWaves workgroups that start together on a CU at the head of a large launch (blocks b, b + 256, b + 512,
// ... with the observed round-robin placement; nothing depends on it) begin 0, 1, 2, ... x kSleepStagger x 64 cycles
// apart (2.6 us steps), so that their load phases do not coincide from the first pass on.  Measured in bench.py
// with four per CU: -3.2 .. -4.0 % kernel time on one MI355X box, +-0.5 % on another; steps of 1.2 us did nothing,
// steps of 3.7 us and more were worse than 2.6.  With five per CU (96 VGPRs since round 4) and only the first four
// staggered the step was 3 % slower than with all five (profiles/r4_ab_runs.txt section 7).
__device__ __forceinline__ void stagger_start()
{
    if (gridDim.x >= 256u * kMinWaves * 4 / kWaves && blockIdx.x < 256u * kMinWaves * 4 / kWaves) {
        const uint32_t slot = blockIdx.x >> 8;
        for (uint32_t i = 0; i < slot; i++)
            __builtin_amdgcn_s_sleep(kSleepStagger);
    }
}

// One tile of any entry: one workgroup of four waves; the planes' pad words, Stage A, a barrier, Stage B between barriers,
// the profile clocks.  `args` are the tile's own (a batch tile's: its segment's samples and offsets), K its passes, t0 its
// first owned offset, prof_begin the clock its entry read behind the stagger (0 without args.profile).
// (Kernel arguments are only ever used by value -- taking their address would demote the sample pointer to a flat / scratch
// access: the reference here disappears with the inlining.)
template <bool kStats, int kFront>
__device__ __forceinline__ void scan_tile(const ScanArgs &args, const int K, const int64_t t0, const uint64_t prof_begin, uint32_t *smem)
{
    const int nplane = kPassRuns * K + kPlanePad;
    uint32_t *pl_d = smem;
    uint32_t *pl_e1 = smem + nplane;
    uint32_t *pl_e2 = smem + 2 * nplane;
    uint32_t *queue = smem + 3 * nplane;
    uint32_t *qcount = queue + kQueueCap;
    uint32_t *cl_rec = qcount + 16; // kClistCap records of kCandWords
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = tid >> 6;

    // plane words past the last computed run are read (never used) by Stage B
    if (tid < kPlanePad) {
        pl_d[kPassRuns * K + tid] = 0;
        pl_e1[kPassRuns * K + tid] = 0;
        pl_e2[kPassRuns * K + tid] = 0;
    }

    ADSB_STAMP_BEGIN();
    if constexpr (kFront == kFrontIq)
        stage_a_iq(args.x, args.pbuf0, args.p_lo, args.p_hi, t0, K, wave, lane, pl_d, pl_e1, pl_e2);
    else if constexpr (kFront == kFrontIq8)
        stage_a_iq8(args.x, args.pbuf0, args.p_lo, args.p_hi, t0, K, wave, lane, pl_d, pl_e1, pl_e2);
    else if constexpr (kFront == kFrontPower)
        stage_a_power(args.x, args.pbuf0, args.p_lo, args.p_hi, t0, K, wave, lane, pl_d, pl_e1, pl_e2);
    else
        stage_a(args.x, args.pbuf0, args.p_lo, args.p_hi, t0, K, wave, lane, pl_d, pl_e1, pl_e2);
    __syncthreads();
    ADSB_STAMP(1); // Stage A
    ADSB_COUNT(0, 1);
    stage_b<kStats, kFront>(args, blockIdx.x, K, t0, tid, pl_d, pl_e1, pl_e2, queue, qcount, cl_rec, args.clist_cap, stamp_last);
    ADSB_STAMP_END(13); // the marker

    if (args.profile) { // the launch's duration is (latest tile end) - (earliest tile start)
        __syncthreads();
        if (tid == 64) { // not wave 0: that one has just issued the tile's write-through stores
            unsigned long long *c64 = reinterpret_cast<unsigned long long *>(args.counters);
            atomicMax(&c64[2 * kCounterPad], ~(unsigned long long)prof_begin); // = counters 4 and 5
            atomicMax(&c64[(5 * kCounterPad) / 2], (unsigned long long)__builtin_amdgcn_s_memrealtime());
        }
    }
}

// Host: the launch behind launch_scan*(): a stream's tiles, kernel `with_stats` or `without`, and the report kernel behind them
inline hipError_t launch_stream_tiles(void (*with_stats)(ScanArgs), void (*without)(ScanArgs), const ScanArgs &args, bool stats,
                                      hipStream_t stream)
{
    if (args.g_end <= args.g_begin)
        return hipSuccess;
    const unsigned blocks = tile_count(args.g_end - args.g_begin, args.big_tiles, args.passes);
    hipLaunchKernelGGL(stats ? with_stats : without, dim3(blocks), dim3(kThreads), lds_bytes(args.passes), stream, args);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : launch_report(args, stream);
}

// ... and behind launch_scan_batch*(): the n_tiles tiles of a batch's segments
using BatchTilesKernel = void (*)(ScanArgs, const BatchSeg *, const uint32_t *);
inline hipError_t launch_batch_tiles(BatchTilesKernel with_stats, BatchTilesKernel without, const ScanArgs &args, const BatchSeg *segs,
                                     const uint32_t *tile_seg, uint32_t n_tiles, bool stats, hipStream_t stream)
{
    if (n_tiles == 0)
        return hipSuccess;
    hipLaunchKernelGGL(stats ? with_stats : without, dim3(n_tiles), dim3(kThreads), lds_bytes(args.passes), stream, args, segs, tile_seg);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : launch_report(args, stream);
}

} // namespace adsb
