// unpack12_batch.hip -- the packed 12-bit captures of a batch (adsb_decode_batch_*_packed) -> uint16 samples, ONE launch for all.
//
// Per group the work is unpack12.hip's: a lane turns 12 bytes (one global_load_dwordx3) into 16 bytes (one
// global_store_dwordx4) through packed12.h's unpack12_group_pairs -- the function the CPU test checks.  No LDS, no scratch.
// What is new is finding the capture a group belongs to.  The groups of all captures are numbered in ONE space, capture after
// capture, and a table of one row per capture THAT HAS GROUPS (Unpack12Seg: source, destination, first group; a capture of 0
// groups has no row and costs nothing) says where a capture's numbers start; a row behind the last one holds the total.
// A block takes chunks of 256 consecutive groups, grid-stride.  Per chunk it searches the table twice, for the rows of the
// chunk's first and last group -- block-uniform values, so these are scalar loads and wave-uniform compares, once per wave, not
// per lane.  Almost always the two rows are the same one (a capture of 1 Mi samples is 512 chunks) and a lane has nothing left to
// look up; where a chunk spans several captures (captures of a few groups side by side) a lane bisects between the two rows
// only.  The table is O(captures): 2 048 captures upload 48 KiB, whatever their lengths, and a capture of 1 group and one of
// 2^29 groups in one launch are two rows.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "packed12.h"

namespace adsb {

__global__ __launch_bounds__(256) void unpack12_batch_kernel(uint16_t *__restrict__ dst, const Unpack12Seg *__restrict__ tab,
                                                             uint32_t n_rows, uint64_t groups)
{
    uint4 *d4 = reinterpret_cast<uint4 *>(dst);
    const uint64_t chunks = (groups + kUnpack12Chunk - 1) / kUnpack12Chunk;
    for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint64_t g0 = c * kUnpack12Chunk, g1 = g0 + (kUnpack12Chunk - 1) < groups ? g0 + (kUnpack12Chunk - 1) : groups - 1;
        const uint32_t r0 = unpack12_row(tab, 0, n_rows - 1, g0); // block-uniform: the scalar unit's
        const uint32_t r1 = unpack12_row(tab, r0, n_rows - 1, g1);
        const uint64_t g = g0 + threadIdx.x;
        if (g > g1)
            continue;
        const uint32_t r = unpack12_row(tab, r0, r1, g); // (r0 == r1: no iteration)
        const uint64_t k = g - tab[r].g_first;           // the group's number inside its capture
        // (an address read from a table is a generic one to the compiler: said to be global memory, the load is a global_load)
        typedef const __attribute__((address_space(1))) uint32_t *global_words;
        const global_words w = (global_words)tab[r].src + 3 * k;
        uint32_t o[4];
        unpack12_group_pairs(w[0], w[1], w[2], o);
        d4[tab[r].dst16 + k] = make_uint4(o[0], o[1], o[2], o[3]);
    }
}

hipError_t launch_unpack12_batch(uint16_t *dst, const Unpack12Seg *tab_device, uint32_t n_rows, uint64_t groups, hipStream_t stream)
{
    if (groups == 0 || n_rows == 0)
        return hipSuccess;
    // as launch_unpack12: 8 blocks of 256 lanes per CU at most (2048 on the 256 CUs of an MI355X) stream HBM
    const unsigned blocks = (unsigned)std::min<uint64_t>(2048, (groups + kUnpack12Chunk - 1) / kUnpack12Chunk);
    hipLaunchKernelGGL(unpack12_batch_kernel, dim3(blocks), dim3(kUnpack12Chunk), 0, stream, dst, tab_device, n_rows, groups);
    return hipGetLastError();
}

} // namespace adsb
