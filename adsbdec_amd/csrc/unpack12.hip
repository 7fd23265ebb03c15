// unpack12.hip -- Airspy packed 12-bit samples (include/adsbdec_amd.h: the format) -> the uint16 samples the scan reads.
//
// A separate, memory-bound pass on purpose: the scan kernel converts uint16 to f32 inside its typed buffer loads at no
// VALU cost, and it is VALU-bound; teaching it the packed layout would put an extract and a convert per sample on that
// path.  Here a lane turns one group (12 bytes in: one global_load_dwordx3; 16 bytes out: one global_store_dwordx4) into
// eight samples with the same function the CPU test checks (packed12.h).  Grid-stride, no LDS, no scratch.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "packed12.h"

namespace adsb {

__global__ __launch_bounds__(256) void unpack12_kernel(uint16_t *__restrict__ dst, const uint32_t *__restrict__ src, size_t groups)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    uint4 *d4 = reinterpret_cast<uint4 *>(dst);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < groups; i += stride) {
        const uint32_t *w = src + 3 * i;
        uint32_t o[4];
        unpack12_group_pairs(w[0], w[1], w[2], o);
        d4[i] = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

hipError_t launch_unpack12(uint16_t *dst, const void *src, size_t groups, hipStream_t stream)
{
    if (groups == 0)
        return hipSuccess;
    // 8 blocks of 256 lanes per CU at most (2048 on the 256 CUs of an MI355X): enough loads in flight to stream HBM
    const unsigned blocks = (unsigned)std::min<size_t>(2048, (groups + 255) / 256);
    hipLaunchKernelGGL(unpack12_kernel, dim3(blocks), dim3(256), 0, stream, dst, static_cast<const uint32_t *>(src), groups);
    return hipGetLastError();
}

} // namespace adsb
