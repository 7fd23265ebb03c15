// burst_kernel.hip -- the gate behind the envelope (include/adsbdec_amd.h: adsb_bursts_*): an envelope of R floats, one per run of
// 28 power samples, -> the ordered table of its bursts.  adsbdec_amd/levels.py bursts is the definition: run r is hot iff
// u[r] >= bits(threshold) as unsigned integers (u: the float's bits, 0 where its sign is set); the hot runs, cut wherever two
// neighbours lie more than join = lead + hang + 1 apart, are the bursts.  Integer work throughout: the table is held to numpy's
// for equality.
//
// A hot run is a START when no hot run precedes it or the previous one lies more than join back, an END when none follows or the
// next lies more than join ahead; burst k runs from the k-th start to the end that follows it.  A tile is kBurstTileRuns
// consecutive runs and one workgroup of 256 lanes, a lane holding eight consecutive runs (two 16-byte loads), a wave 512.
// Three kernels, one behind the other on ONE stream; the stream is the only ordering there is:
//   burst_summary_kernel   a workgroup per tile -> {first hot run, last hot run, starts strictly inside the tile}
//   burst_combine_kernel   ONE workgroup walks the summaries -- backwards for every tile's next hot run, forwards for its
//                          previous one and the starts before it -- and leaves a row per tile, and B
//   burst_emit_kernel      a workgroup per tile that has a hot run redoes its hot runs with the row's four words in hand
// NO WORKGROUP EVER WAITS FOR ANOTHER: no look-back, no flag that is polled, no grid barrier.  What a tile needs of its neighbours
// is in memory before its kernel starts.
//
// Inside a wave the previous hot run of a lane is found from the ballot of "this lane has a hot run": the mask below the lane, a
// count of leading zeros, one shuffle of that lane's last hot run; the next one likewise from the mask above and its trailing
// zeros.  The four waves of a tile meet in LDS (one barrier in the summary kernel, two in the emit).
//
// Stores: begin and end of a record are plain vector stores by the one hot run that is the burst's start / end; hot and peak are
// written by vector atomics only, into a table the host zeroed on the same stream (a start that stored hot = 0 would race with the
// other tiles of its burst).  A lane adds a burst's hot runs among its eight at once, and a wave whose lanes all hold the same
// burst adds once for all of them: an envelope that is one long burst costs an atomic pair per 512 runs, not per run.
// The kernels are burst_tile.h's, shared with the gate of a slice of a stream (burst_slice_kernel.hip).
#define ADSB_BURST_SLICE 0
#include "burst_tile.h"

namespace adsb {

hipError_t launch_burst_count(const BurstArgs &a, hipStream_t stream)
{
    if (a.n_tiles == 0)
        return hipSuccess;
    hipLaunchKernelGGL(burst_summary_kernel, dim3(a.n_tiles), dim3(kLanes), 0, stream, a);
    hipLaunchKernelGGL(burst_combine_kernel, dim3(1), dim3(kLanes), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_burst_emit(const BurstArgs &a, hipStream_t stream)
{
    if (a.n_tiles == 0 || a.cap == 0)
        return hipSuccess;
    hipLaunchKernelGGL(burst_emit_kernel, dim3(a.n_tiles), dim3(kLanes), 0, stream, a);
    return hipGetLastError();
}

} // namespace adsb
