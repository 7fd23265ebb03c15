// burst_slice_kernel.hip -- the gate of a SLICE of a stream (include/adsbdec_amd.h: adsb_bursts_slice_*; decoder_bursts.hip):
// n_env floats that continue the runs earlier calls covered, and the cluster those calls left open, -> the clusters of the slice
// in stream runs.  adsbdec_amd/levels.py bursts_slice is the definition.  The three kernels are burst_kernel.hip's, on one stream
// and with no workgroup waiting for another; burst_tile.h states what they do and where a slice differs (ADSB_BURST_SLICE):
//   the summaries   hold stream runs
//   the combine     takes the carried cluster's last hot run as the hot run before tile 0 and the cluster as the one start in
//                   front of the slice: a hot run within join of it is no start, and B counts the carried cluster
//   the emit        writes unclipped ends, and the last cluster -- the only one that can stay open -- with its TRUE first and last
//                   hot run behind the records the caller has room for
// What is left to the host is two records (decoder_bursts.hip): the carried cluster's begin, count and peak into burst 0, and the
// last burst into the table or into the carry.
#define ADSB_BURST_SLICE 1
#include "burst_tile.h"

namespace adsb {

hipError_t launch_burst_slice_count(const BurstArgs &a, const BurstSlice &s, hipStream_t stream)
{
    if (a.n_tiles == 0)
        return hipSuccess;
    hipLaunchKernelGGL(burst_slice_summary_kernel, dim3(a.n_tiles), dim3(kLanes), 0, stream, a, s);
    hipLaunchKernelGGL(burst_slice_combine_kernel, dim3(1), dim3(kLanes), 0, stream, a, s);
    return hipGetLastError();
}

hipError_t launch_burst_slice_emit(const BurstArgs &a, const BurstSlice &s, hipStream_t stream)
{
    if (a.n_tiles == 0)
        return hipSuccess;
    hipLaunchKernelGGL(burst_slice_emit_kernel, dim3(a.n_tiles), dim3(kLanes), 0, stream, a, s);
    return hipGetLastError();
}

} // namespace adsb
