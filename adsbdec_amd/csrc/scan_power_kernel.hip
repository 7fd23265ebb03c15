// scan_power_kernel.hip -- the scan kernels for a stream of float32 POWER samples at 10 MS/s (DESIGN.md "Power samples"), for
// gfx950.  The stream is the reference's `ampbuff` itself (adsbdec.h:5: deqframe(const float *ampbuff, const int len)): the
// caller's front end -- another SDR, a filter of their own, a tensor computed on the GPU -- has done everything that comes
// before it, and everything behind it is the reference's demodulator unchanged: Stage A's plane arithmetic and all of Stage B
// are the code of scan_stages.h that the other scan units run.  What is this unit's own is the front end (stage_a_power:
// seven 16-byte loads per run, nothing computed) and pw's four loads (pw_at_power).  A power sample is 4 bytes, as a complex
// int16 sample is: ScanArgs, the tile geometry, the LDS, the hand-off stream and the count pass are scan_iq_kernel's, with x
// the floats and pbuf0 / p_lo / p_hi their indices.
//
// Input domain (include/adsbdec_amd.h): finite, sign bit clear, below 2^29; subnormals included -- stage_a_power says where
// that matters.  Outside it the reference itself is undefined behaviour and nothing is promised here.
//
// A translation unit of its own: tests/test_build_flags.py counts the kernels and the fused operations of scan_kernel.hip's.
// The only fused operations here are the sign tests of the plane arithmetic (-ffp-contract=off).
#undef ADSB_PHASE_STAMPS // (a measurement build's per-phase clocks, scan_stamps.h, are scan_kernel.hip's alone)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_kernel.h"
#include "scan_stages.h"
#include "scan_tile.h" // the tile shell, the stagger, the launchers (after scan_stages.h: see there)

namespace adsb {

// scan_kernel for power samples: the tiles partition one stream
template <bool kStats>
__global__ __launch_bounds__(kThreads, kMinWaves) void scan_power_kernel(const ScanArgs args)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const int K = tile_passes(blockIdx.x, args.big_tiles, args.passes);
    stagger_start();
    const uint64_t prof_begin = args.profile ? __builtin_amdgcn_s_memrealtime() : 0;
    const int64_t t0 = // first owned offset
        (int64_t)args.g_begin + (int64_t)kRun * (int64_t)tile_first_run(blockIdx.x, args.big_tiles, args.passes);
    scan_tile<kStats, kFrontPower>(args, K, t0, prof_begin, smem);
}

// scan_batch_kernel for power samples: the tiles belong to the captures of a batch (scan_kernel.h BatchSeg)
template <bool kStats>
__global__ __launch_bounds__(kThreads, kMinWaves) void scan_power_batch_kernel(const ScanArgs launch, const BatchSeg *__restrict__ segs,
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
    scan_tile<kStats, kFrontPower>(args, K, t0, prof_begin, smem);
}

hipError_t launch_scan_power(const ScanArgs &args, bool stats, hipStream_t stream)
{
    return launch_stream_tiles(scan_power_kernel<true>, scan_power_kernel<false>, args, stats, stream);
}

hipError_t launch_scan_batch_power(const ScanArgs &args, const BatchSeg *segs, const uint32_t *tile_seg, uint32_t n_tiles, bool stats,
                                   hipStream_t stream)
{
    return launch_batch_tiles(scan_power_batch_kernel<true>, scan_power_batch_kernel<false>, args, segs, tile_seg, n_tiles, stats, stream);
}

} // namespace adsb
