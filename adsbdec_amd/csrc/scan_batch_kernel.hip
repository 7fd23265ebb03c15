// scan_batch_kernel.hip -- the scan kernel for a batch of independent captures: one launch whose tiles belong to different
// captures (adsb_decode_batch_*; DESIGN.md "Batches of captures").  The same two stages as scan_kernel (scan_stages.h), the
// same launch bounds, the same dynamic LDS; what differs is where a workgroup gets its samples and its offsets from: it
// looks its SEGMENT up in a device table (scan_kernel.h BatchSeg) and runs the stages with that segment's values.
#undef ADSB_PHASE_STAMPS // (a measurement build's per-phase clocks, scan_stamps.h, are scan_kernel.hip's alone)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "scan_kernel.h"
#include "scan_stages.h"
#include "scan_tile.h" // the stagger, the launcher (after scan_stages.h: see there)

namespace adsb {

template <bool kStats>
__global__ __launch_bounds__(kThreads, kMinWaves) void scan_batch_kernel(const ScanArgs launch, const BatchSeg *__restrict__ segs,
                                                                         const uint32_t *__restrict__ tile_seg)
{
    // The tile shell in this kernel's own lines, not scan_tile's (scan_tile.h): over scan_tile the <false> instantiation's scalar
    // registers are renamed inside Stage B's loops (profiles/r31_tile_shell_isa_identity.txt).  The stagger and the launcher are shared.
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const int K = launch.passes; // one K per launch, no taper
    const int nplane = kPassRuns * K + kPlanePad;
    uint32_t *pl_d = smem;
    uint32_t *pl_e1 = smem + nplane;
    uint32_t *pl_e2 = smem + 2 * nplane;
    uint32_t *queue = smem + 3 * nplane;
    uint32_t *qcount = queue + kQueueCap;
    uint32_t *cl_rec = qcount + 16; // kClistCap records of kCandWords

    const int tid = threadIdx.x;
    stagger_start();
    const uint64_t prof_begin = launch.profile ? __builtin_amdgcn_s_memrealtime() : 0;
    const int lane = tid & 63;
    const int wave = tid >> 6;

    // The workgroup's segment: workgroup-uniform loads (scalar ones) of a table word and of the segment's 56 bytes.  The sample
    // pointer now comes from memory, where the compiler cannot know its address space: said here, so that Stage B's plain
    // loads of samples (pw_load) stay global loads.  (Stage A builds a buffer resource from it.)
    const BatchSeg sg = segs[tile_seg[blockIdx.x]];
    ScanArgs args = launch; // by value, its address is never taken: the members stay in registers (scan_kernel's note)
    args.x = (const uint32_t *)(const __attribute__((address_space(1))) uint32_t *)(uintptr_t)sg.x;
    args.pbuf0 = sg.pbuf0;
    args.p_lo = sg.p_lo;
    args.p_hi = sg.p_hi;
    args.g_end = sg.g_end; // the tile's offsets end with the segment's; g_rel still counts from the LAUNCH's g_begin
    const int64_t t0 = // first owned offset
        (int64_t)sg.g_begin + (int64_t)kRun * (int64_t)tile_first_run(blockIdx.x - sg.first_tile, 0u, K);

    // plane words past the last computed run are read (never used) by Stage B
    if (tid < kPlanePad) {
        pl_d[kPassRuns * K + tid] = 0;
        pl_e1[kPassRuns * K + tid] = 0;
        pl_e2[kPassRuns * K + tid] = 0;
    }

    uint64_t stamp_last = 0;
    stage_a(args.x, args.pbuf0, args.p_lo, args.p_hi, t0, K, wave, lane, pl_d, pl_e1, pl_e2);
    __syncthreads();
    stage_b<kStats>(args, blockIdx.x, K, t0, tid, pl_d, pl_e1, pl_e2, queue, qcount, cl_rec, args.clist_cap, stamp_last);

    if (launch.profile) { // the launch's duration is (latest tile end) - (earliest tile start)
        __syncthreads();
        if (tid == 64) {
            unsigned long long *c64 = reinterpret_cast<unsigned long long *>(launch.counters);
            atomicMax(&c64[2 * kCounterPad], ~(unsigned long long)prof_begin); // = counters 4 and 5
            atomicMax(&c64[(5 * kCounterPad) / 2], (unsigned long long)__builtin_amdgcn_s_memrealtime());
        }
    }
}

hipError_t launch_scan_batch(const ScanArgs &args, const BatchSeg *segs, const uint32_t *tile_seg, uint32_t n_tiles, bool stats,
                             hipStream_t stream)
{
    return launch_batch_tiles(scan_batch_kernel<true>, scan_batch_kernel<false>, args, segs, tile_seg, n_tiles, stats, stream);
}

} // namespace adsb
