// gather_pack12_kernel.hip -- a real capture's bursts, piece after piece, PACKED to 12 bits while they are copied, into ONE array
// (adsb_gather_pack12_*; gather_pack12.h has the layout), ONE launch.  The shape is gather_kernel.hip's:
//
// The output is numbered in 16-byte words across all pieces, and a table of one row per piece (GatherPack12Row: first word, source
// sample offset, samples, own samples; a row behind the last holds the total) says where a piece's words start.  A block takes
// chunks of 256 consecutive words, grid-stride.  Per chunk it searches the table twice, for the rows of the chunk's first and last
// word -- block-uniform values, so these are scalar loads and wave-uniform compares, once per wave.  Where the two rows are one a
// lane has nothing to look up; where a chunk spans several pieces a lane bisects between the two rows only.  A lane stores 16
// bytes, always: consecutive lanes write consecutive words.
//
// Word k of a piece starts at packed byte 16 k = 12 j + 4 d, d = k % 3, j = (4 k - d) / 3: it is the dwords d .. 2 of group j, then
// the dwords 0 .. d of group j + 1.  A lane therefore reads at most two groups, each ONE 16-byte aligned load of 8 codes (a piece
// starts at sample 56 begin, a multiple of 8, in a 16-byte aligned capture).  Nothing outside the piece's own samples
// [src, src + own) is read: a last half group (own = samples - 4, a last piece that M clips with M % 4 == 2) is read as 8 bytes and
// its four missing codes are 2048; a group at or behind samples / 8 is not read and gives zero bytes, the pad of the piece's last
// word.  Every offset is 64-bit.
//
// `over`: the own samples above 4095, counted once each by the lane whose word holds the group's first byte -- group j + 1 always
// (its byte 0 is this word's byte 12 - 4 d), group j where d == 0 -- and added by one vector atomic per lane that has any (almost
// none on a capture whose codes are 12-bit) to a word the caller zeroed on the same stream.  No LDS, no scratch.
//
// Four groups feed three words, so a group is loaded 1.5 times on average.  -DADSB_GATHER_PACK12_LANE3=1 builds the other form that
// the plan wanted measured beside this one: a lane that loads four groups once each and stores three words, 48 bytes apart from its
// neighbour's (tools/format_probe.py --gather-pack12 --variant name=lib; DESIGN.md "Burst archive at 12 bits").
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gather_pack12.h"
#include "packed12.h"

namespace adsb {

namespace {

// The last row of tab[lo .. hi] whose first word is <= w (tab[lo].w_first <= w is the caller's).
__device__ inline uint32_t pack12_row(const GatherPack12Row *tab, uint32_t lo, uint32_t hi, uint64_t w)
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

// Group g of the piece whose samples start at `src` (16-byte aligned), `groups` groups of which the first `own` samples exist:
// its three packed dwords in w, zero where g >= groups; returns its own samples above 4095.
__device__ __forceinline__ uint32_t pack12_load(const uint16_t *src, uint64_t g, uint64_t groups, uint64_t own, uint32_t (&w)[3])
{
    w[0] = w[1] = w[2] = 0;
    if (g >= groups)
        return 0;
    constexpr uint32_t kFill2 = kPack12Fill | (kPack12Fill << 16);
    uint4 q;
    if (8 * g + 8 <= own) {
        q = *reinterpret_cast<const uint4 *>(src + 8 * g);
    } else { // the half group of a clipped last piece: own - 8 g == 4
        const uint2 a = *reinterpret_cast<const uint2 *>(src + 8 * g);
        q = make_uint4(a.x, a.y, kFill2, kFill2);
    }
    const uint32_t p[4] = {q.x, q.y, q.z, q.w};
    uint16_t s[8];
    uint32_t n_over = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        s[2 * k] = (uint16_t)p[k];
        s[2 * k + 1] = (uint16_t)(p[k] >> 16);
        n_over += ((p[k] & 0xF000u) != 0) + ((p[k] >> 28) != 0); // (the fill is 2048: never counted)
    }
    pack12_group(s, w);
    return n_over;
}

#if ADSB_GATHER_PACK12_LANE3
// The measurement build: the output numbered in TRIPLES of words across all pieces (a piece of G groups has ceil(G / 4) of them), a
// lane loads the four groups 4 t .. 4 t + 3 of its triple t once each and stores the words 3 t .. 3 t + 2 that the piece has -- no
// group is loaded twice, and a wave's three stores are each 48 bytes apart from lane to lane.  `words` is the number of all triples.
__global__ __launch_bounds__(256) void gather_pack12_kernel(uint4 *__restrict__ out, const uint16_t *__restrict__ capture,
                                                            const GatherPack12Row *__restrict__ tab, uint32_t n_rows, uint64_t words,
                                                            unsigned long long *__restrict__ over)
{
    auto row = [tab](uint32_t lo, uint32_t hi, uint64_t t) {
        while (lo < hi) {
            const uint32_t mid = lo + (hi - lo + 1) / 2;
            if (tab[mid].t_first <= t)
                lo = mid;
            else
                hi = mid - 1;
        }
        return lo;
    };
    const uint64_t chunks = (words + kGatherChunk - 1) / kGatherChunk;
    for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint64_t t0 = c * kGatherChunk, t1 = t0 + (kGatherChunk - 1) < words ? t0 + (kGatherChunk - 1) : words - 1;
        const uint32_t r0 = row(0, n_rows - 1, t0); // block-uniform
        const uint32_t r1 = row(r0, n_rows - 1, t1);
        const uint64_t t = t0 + threadIdx.x;
        if (t > t1)
            continue;
        const uint32_t r = row(r0, r1, t);
        const uint64_t k = t - tab[r].t_first;                          // the triple inside its piece
        const uint64_t groups = tab[r].samples / 8, own = tab[r].own;
        const uint64_t piece_words = tab[r + 1].w_first - tab[r].w_first; // (row r + 1 exists: the closing row at least)
        const uint16_t *src = capture + tab[r].src;
        uint32_t g[4][3], mine = 0;
#pragma unroll
        for (int i = 0; i < 4; i++)
            mine += pack12_load(src, 4 * k + i, groups, own, g[i]);
        const uint4 v[3] = {make_uint4(g[0][0], g[0][1], g[0][2], g[1][0]), make_uint4(g[1][1], g[1][2], g[2][0], g[2][1]),
                            make_uint4(g[2][2], g[3][0], g[3][1], g[3][2])};
        uint4 *dst = out + tab[r].w_first + 3 * k;
#pragma unroll
        for (int i = 0; i < 3; i++)
            if (3 * k + i < piece_words)
                dst[i] = v[i];
        if (mine)
            atomicAdd(over, (unsigned long long)mine);
    }
}
#else
__global__ __launch_bounds__(256) void gather_pack12_kernel(uint4 *__restrict__ out, const uint16_t *__restrict__ capture,
                                                            const GatherPack12Row *__restrict__ tab, uint32_t n_rows, uint64_t words,
                                                            unsigned long long *__restrict__ over)
{
    const uint64_t chunks = (words + kGatherChunk - 1) / kGatherChunk;
    for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint64_t w0 = c * kGatherChunk, w1 = w0 + (kGatherChunk - 1) < words ? w0 + (kGatherChunk - 1) : words - 1;
        const uint32_t r0 = pack12_row(tab, 0, n_rows - 1, w0); // block-uniform: the scalar unit's
        const uint32_t r1 = pack12_row(tab, r0, n_rows - 1, w1);
        const uint64_t w = w0 + threadIdx.x;
        if (w > w1)
            continue;
        const uint32_t r = pack12_row(tab, r0, r1, w); // (r0 == r1: no iteration)
        const uint64_t k = w - tab[r].w_first;         // the word inside its piece
        const uint32_t d = (uint32_t)(k % 3);
        const uint64_t j = (4 * k - d) / 3;
        const uint64_t groups = tab[r].samples / 8, own = tab[r].own;
        const uint16_t *src = capture + tab[r].src;
        uint32_t a[3], b[3];
        const uint32_t over_a = pack12_load(src, j, groups, own, a); // (j < groups: a piece has ceil(12 groups / 16) words)
        const uint32_t over_b = pack12_load(src, j + 1, groups, own, b);
        uint4 v;
        if (d == 0)
            v = make_uint4(a[0], a[1], a[2], b[0]);
        else if (d == 1)
            v = make_uint4(a[1], a[2], b[0], b[1]);
        else
            v = make_uint4(a[2], b[0], b[1], b[2]);
        out[w] = v;
        const uint32_t mine = over_b + (d == 0 ? over_a : 0u);
        if (mine)
            atomicAdd(over, (unsigned long long)mine);
    }
}
#endif

} // namespace

hipError_t launch_gather_pack12(void *out, const uint16_t *capture, const GatherPack12Row *tab_device, uint32_t n_rows, uint64_t words,
                                unsigned long long *over, hipStream_t stream)
{
    if (words == 0 || n_rows == 0)
        return hipSuccess;
    // as launch_gather: 8 blocks of 256 lanes per CU at most (2048 on the 256 CUs of an MI355X) stream HBM
    const unsigned blocks = (unsigned)std::min<uint64_t>(2048, (words + kGatherChunk - 1) / kGatherChunk);
    hipLaunchKernelGGL(gather_pack12_kernel, dim3(blocks), dim3(kGatherChunk), 0, stream, static_cast<uint4 *>(out), capture, tab_device,
                       n_rows, words, over);
    return hipGetLastError();
}

} // namespace adsb
