// scan_iq8_kernel.hip -- the scan kernels for a stream of COMPLEX int8 samples at 10 MS/s (interleaved signed bytes I, Q: HackRF
// cs8, bladeRF / USRP sc8; DESIGN.md "int8 IQ captures"), for gfx950.  An int8 stream is decoded as the int16 IQ stream
// (I << 8, Q << 8) is: power sample m is 256 (I^2 + Q^2) of sample m, an exact integer, and everything behind the power samples is
// the reference's demodulator unchanged -- Stage A's plane arithmetic and all of Stage B are the code of scan_stages.h that the
// other scan kernels run.  What is this unit's own is the front end (stage_a_iq8: fourteen typed 4-byte loads, 28 products and 14
// sums, all packed, per run) and pw's four 2-byte loads (pw_at_iq8).  A complex sample is 2 bytes: ScanArgs, the tile geometry in samples, the LDS,
// the hand-off stream and the count pass are scan_kernel's, with x addressed in 2-byte complex samples and pbuf0 / p_lo / p_hi their
// indices.  The first sample of the buffer must be 8-byte aligned and pbuf0 a multiple of 4.
//
// A translation unit of its own: tests/test_build_flags.py counts the kernels and the fused operations of scan_kernel.hip's.
// The only fused float operations here are the sign tests of the plane arithmetic.
#undef ADSB_PHASE_STAMPS // (a measurement build's per-phase clocks, scan_stamps.h, are scan_kernel.hip's alone)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_kernel.h"
#include "scan_stages.h"
#include "scan_tile.h" // the tile shell, the stagger, the launchers (after scan_stages.h: see there)

namespace adsb {

// scan_kernel for complex int8 samples: the tiles partition one stream
template <bool kStats>
__global__ __launch_bounds__(kThreads, kMinWaves) void scan_iq8_kernel(const ScanArgs args)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const int K = tile_passes(blockIdx.x, args.big_tiles, args.passes);
    stagger_start();
    const uint64_t prof_begin = args.profile ? __builtin_amdgcn_s_memrealtime() : 0;
    const int64_t t0 = // first owned offset
        (int64_t)args.g_begin + (int64_t)kRun * (int64_t)tile_first_run(blockIdx.x, args.big_tiles, args.passes);
    scan_tile<kStats, kFrontIq8>(args, K, t0, prof_begin, smem);
}

// scan_batch_kernel for complex int8 samples: the tiles belong to the captures of a batch (scan_kernel.h BatchSeg)
template <bool kStats>
__global__ __launch_bounds__(kThreads, kMinWaves) void scan_iq8_batch_kernel(const ScanArgs launch, const BatchSeg *__restrict__ segs,
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
    scan_tile<kStats, kFrontIq8>(args, K, t0, prof_begin, smem);
}

hipError_t launch_scan_iq8(const ScanArgs &args, bool stats, hipStream_t stream)
{
    return launch_stream_tiles(scan_iq8_kernel<true>, scan_iq8_kernel<false>, args, stats, stream);
}

hipError_t launch_scan_batch_iq8(const ScanArgs &args, const BatchSeg *segs, const uint32_t *tile_seg, uint32_t n_tiles, bool stats,
                                 hipStream_t stream)
{
    return launch_batch_tiles(scan_iq8_batch_kernel<true>, scan_iq8_batch_kernel<false>, args, segs, tile_seg, n_tiles, stats, stream);
}

} // namespace adsb
