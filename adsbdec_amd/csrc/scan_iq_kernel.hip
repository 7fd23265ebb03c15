// scan_iq_kernel.hip -- the scan kernels for a stream of COMPLEX int16 samples at 10 MS/s (airspy_rx -t 2; DESIGN.md
// "IQ captures"), for gfx950.  libairspy has already done what the FIR of scan_kernel.hip does -- the fs/4 mix, the half-band
// filter, the decimation -- so power sample m is |sample m|^2 and everything behind the power samples is the reference's
// demodulator unchanged: Stage A's plane arithmetic and all of Stage B are the code of scan_stages.h that scan_kernel and
// scan_batch_kernel run.  What is this unit's own is the front end (stage_a_iq: typed signed loads, 56 products and 28 sums
// per run) and pw's four loads (pw_at_iq).  A complex sample is 4 bytes, as the (I, Q) pair of real samples behind one power
// sample is: ScanArgs, the tile geometry, the LDS, the hand-off stream and the count pass are scan_kernel's, with x the
// complex samples and pbuf0 / p_lo / p_hi their indices.
//
// A translation unit of its own: tests/test_build_flags.py counts the kernels and the fused operations of scan_kernel.hip's.
// The arithmetic is binary32 multiply, then add (-ffp-contract=off); the only fused operations here are the sign tests of
// the plane arithmetic.
#undef ADSB_PHASE_STAMPS // (a measurement build's per-phase clocks, scan_stamps.h, are scan_kernel.hip's alone)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_kernel.h"
#include "scan_stages.h"
#include "scan_tile.h" // the tile shell, the stagger, the launchers (after scan_stages.h: see there)

namespace adsb {

// scan_kernel for complex samples: the tiles partition one stream
template <bool kStats>
__global__ __launch_bounds__(kThreads, kMinWaves) void scan_iq_kernel(const ScanArgs args)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const int K = tile_passes(blockIdx.x, args.big_tiles, args.passes);
    stagger_start();
    const uint64_t prof_begin = args.profile ? __builtin_amdgcn_s_memrealtime() : 0;
    const int64_t t0 = // first owned offset
        (int64_t)args.g_begin + (int64_t)kRun * (int64_t)tile_first_run(blockIdx.x, args.big_tiles, args.passes);
    scan_tile<kStats, kFrontIq>(args, K, t0, prof_begin, smem);
}

// scan_batch_kernel for complex samples: the tiles belong to the captures of a batch (scan_kernel.h BatchSeg)
template <bool kStats>
__global__ __launch_bounds__(kThreads, kMinWaves) void scan_iq_batch_kernel(const ScanArgs launch, const BatchSeg *__restrict__ segs,
                                                                            const uint32_t *__restrict__ tile_seg)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const int K = launch.passes; // one K per launch, no taper
    stagger_start();
    const uint64_t prof_begin = launch.profile ? __builtin_amdgcn_s_memrealtime() : 0;
    const BatchSeg sg = segs[tile_seg[blockIdx.x]];
    ScanArgs args = launch; // by value, its address is never taken (scan_batch_kernel's notes)
    args.x = (const uint32_t *)(const __attribute__((address_space(1))) uint32_t *)(uintptr_t)sg.x;
    args.pbuf0 = sg.pbuf0;
    args.p_lo = sg.p_lo;
    args.p_hi = sg.p_hi;
    args.g_end = sg.g_end;
    const int64_t t0 = (int64_t)sg.g_begin + (int64_t)kRun * (int64_t)tile_first_run(blockIdx.x - sg.first_tile, 0u, K);
    scan_tile<kStats, kFrontIq>(args, K, t0, prof_begin, smem);
}

hipError_t launch_scan_iq(const ScanArgs &args, bool stats, hipStream_t stream)
{
    return launch_stream_tiles(scan_iq_kernel<true>, scan_iq_kernel<false>, args, stats, stream);
}

hipError_t launch_scan_batch_iq(const ScanArgs &args, const BatchSeg *segs, const uint32_t *tile_seg, uint32_t n_tiles, bool stats,
                                hipStream_t stream)
{
    return launch_batch_tiles(scan_iq_batch_kernel<true>, scan_iq_batch_kernel<false>, args, segs, tile_seg, n_tiles, stats, stream);
}

} // namespace adsb
