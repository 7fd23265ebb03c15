// gather_kernel.hip -- a capture's bursts, piece after piece, into ONE array (adsb_gather_device; gather.h has the layout), ONE launch.
//
// The output is numbered in 16-byte words across all pieces, and a table of one row per piece (GatherRow: first word, source byte
// offset, bytes; a row behind the last holds the total) says where a piece's words start.  A block takes chunks of 256 consecutive
// words, grid-stride.  Per chunk it searches the table twice, for the rows of the chunk's first and last word -- block-uniform
// values, so these are scalar loads and wave-uniform compares, once per wave (the shape of unpack12_batch.hip).  Where the two
// rows are one (a chunk inside a long piece) a lane has nothing to look up; where a chunk spans several pieces a lane bisects
// between the two rows only.
//
// A lane stores 16 bytes, always: consecutive lanes write consecutive words, so a wave's store is 1 KiB of whole lines whatever
// the pieces are.  A piece starts at s 28 begin bytes: a multiple of 16 for s = 4 and 8, and for s = 2 a multiple of 16 (begin
// even) or 8 bytes behind one (begin odd).  A full word is ONE 16-byte load told of 8-byte alignment only, whichever the source
// is: the hardware takes it at any dword.  -DADSB_GATHER_LOAD=0 builds the other form that was measured -- aligned: one 16-byte
// load; 8 behind: two 8-byte loads -- which was nowhere ahead (profiles/r32_gather.txt; DESIGN.md "Burst archive").  A piece's
// LAST word is read only as far as the piece reaches -- 8 bytes at once where it has them, then two bytes at a time (a sample is
// 2 bytes at least) -- and the rest of the word is zero: nothing outside [src, src + bytes) is read, so nothing behind the
// capture's last power sample is.  Every offset is 64-bit.  No LDS, no scratch, plain loads and stores
// (profiles/r17_power_export.txt: non-temporal stores buy nothing on this path).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gather.h"

#ifndef ADSB_GATHER_LOAD
#define ADSB_GATHER_LOAD 1 // 1: one 16-byte load at 8-byte alignment; 0 (a measurement build): 16 where aligned, else two 8-byte loads
#endif

namespace adsb {

namespace {

// The last row of tab[lo .. hi] whose first word is <= w (tab[lo].w_first <= w is the caller's).
__device__ inline uint32_t gather_row(const GatherRow *tab, uint32_t lo, uint32_t hi, uint64_t w)
{
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (tab[mid].w_first <= w)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

typedef uint32_t Quad8 __attribute__((ext_vector_type(4), aligned(8))); // 16 bytes known to be 8-byte aligned only

__global__ __launch_bounds__(256) void gather_kernel(uint4 *__restrict__ out, const unsigned char *__restrict__ capture,
                                                     const GatherRow *__restrict__ tab, uint32_t n_rows, uint64_t words)
{
    const uint64_t chunks = (words + kGatherChunk - 1) / kGatherChunk;
    for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint64_t w0 = c * kGatherChunk, w1 = w0 + (kGatherChunk - 1) < words ? w0 + (kGatherChunk - 1) : words - 1;
        const uint32_t r0 = gather_row(tab, 0, n_rows - 1, w0); // block-uniform: the scalar unit's
        const uint32_t r1 = gather_row(tab, r0, n_rows - 1, w1);
        const uint64_t w = w0 + threadIdx.x;
        if (w > w1)
            continue;
        const uint32_t r = gather_row(tab, r0, r1, w); // (r0 == r1: no iteration)
        const uint64_t at = 16 * (w - tab[r].w_first); // the word's first byte inside its piece
        const uint64_t left = tab[r].bytes - at;       // > 0: a piece has ceil(bytes / 16) words
        const unsigned char *src = capture + tab[r].src + at;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (left >= 16) {
#if ADSB_GATHER_LOAD
            const Quad8 q = *reinterpret_cast<const Quad8 *>(src); // at whatever the source's alignment is: 8 bytes at least
            v = make_uint4(q.x, q.y, q.z, q.w);
#else
            if ((tab[r].src & 8) == 0) {
                v = *reinterpret_cast<const uint4 *>(src);
            } else {
                uint32_t upper = 8;
                asm("" : "+v"(upper)); // (kept apart: the compiler otherwise folds the two into a 12-byte load and a dword shared with the aligned path)
                const uint2 a = *reinterpret_cast<const uint2 *>(src), b = *reinterpret_cast<const uint2 *>(src + upper);
                v = make_uint4(a.x, a.y, b.x, b.y);
            }
#endif
        } else { // the piece's last word, short of 16 bytes: `left` is even and below 16
            uint32_t t[4] = {0, 0, 0, 0};
            unsigned have = 0;
            if (left >= 8) {
                const uint2 a = *reinterpret_cast<const uint2 *>(src);
                t[0] = a.x, t[1] = a.y;
                have = 8;
            }
            for (unsigned k = have; k + 2 <= (unsigned)left; k += 2)
                t[k / 4] |= (uint32_t) * reinterpret_cast<const uint16_t *>(src + k) << (8 * (k % 4));
            v = make_uint4(t[0], t[1], t[2], t[3]);
        }
        out[w] = v;
    }
}

} // namespace

hipError_t launch_gather(void *out, const void *capture, const GatherRow *tab_device, uint32_t n_rows, uint64_t words, hipStream_t stream)
{
    if (words == 0 || n_rows == 0)
        return hipSuccess;
    // as launch_unpack12_batch: 8 blocks of 256 lanes per CU at most (2048 on the 256 CUs of an MI355X) stream HBM
    const unsigned blocks = (unsigned)std::min<uint64_t>(2048, (words + kGatherChunk - 1) / kGatherChunk);
    hipLaunchKernelGGL(gather_kernel, dim3(blocks), dim3(kGatherChunk), 0, stream, static_cast<uint4 *>(out),
                       static_cast<const unsigned char *>(capture), tab_device, n_rows, words);
    return hipGetLastError();
}

} // namespace adsb
