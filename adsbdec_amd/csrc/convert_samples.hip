// convert_samples.hip -- signed 16-bit real and float32 real samples (include/adsbdec_amd.h: the formats) -> the uint16 samples the
// scan reads (and the float32 scalars of FLOAT32_IQ -> the int16 scalars the IQ scan reads: one more instantiation), and a count of the samples that do not lie on their format's grid.
//
// A separate, memory-bound pass for unpack12.hip's reason: the scan kernel converts uint16 to f32 inside its typed buffer loads
// at no VALU cost, and it is VALU-bound.  (Scaling float input into the FIR instead would not even be exact: DESIGN.md section 4.)
// A lane turns a group of 8 samples (int16: 16 bytes in; float32: 2 x 16 bytes in) into one 16-byte store with the functions the
// CPU test checks (sample_format.h).  dst may start anywhere (a host push lands at the staging buffer's fill): up to 7 head
// samples bring it to a 16-byte boundary, whole groups follow, then a tail of up to 7.  The source of the groups is then
// aligned to its element only, which the loads say (memcpy from a pointer to the element): no 16-byte alignment is assumed.
// (float32: a wave takes its 64 groups' 2 KiB as consecutive 16-byte pieces and the lanes of a pair swap halves, see
// convert_wave_of_groups.)  Grid-stride; no scratch; LDS: the 8 words of the block's count reduction.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "sample_format.h"

namespace adsb {

namespace {

template <int FMT> struct Element;
template <> struct Element<kFmtInt16Real> { typedef uint16_t type; };
template <> struct Element<kFmtFloat32Real> { typedef uint32_t type; };
template <> struct Element<kConvFloat32Iq> { typedef uint32_t type; };

typedef const __attribute__((address_space(1))) uint16_t *global_u16;
typedef const __attribute__((address_space(1))) uint32_t *global_u32;
template <int FMT> struct GlobalElement;
template <> struct GlobalElement<kFmtInt16Real> { typedef global_u16 type; };
template <> struct GlobalElement<kFmtFloat32Real> { typedef global_u32 type; };
template <> struct GlobalElement<kConvFloat32Iq> { typedef global_u32 type; };

struct Counts {
    uint32_t inexact = 0, clamped = 0;
    __device__ void add(uint32_t what)
    {
        inexact += what == kSampleInexact;
        clamped += what == kSampleClamped;
    }
};

template <int FMT, class P> __device__ inline uint16_t convert_one(P p, Counts &c)
{
    uint32_t what;
    const uint32_t code = sample_code<FMT>(*p, &what);
    c.add(what);
    return (uint16_t)code;
}

// 8 samples at p (aligned to the element, no more) -> the four dwords of their store, sample 2k in the low half of dword k
template <int FMT, class P> __device__ inline uint4 convert_group(P p, Counts &c)
{
    typename Element<FMT>::type e[8];
    __builtin_memcpy(e, p, sizeof e);
    uint32_t o[4];
    for (int k = 0; k < 4; k++) {
        uint32_t w0, w1;
        const uint32_t lo = sample_code<FMT>(e[2 * k], &w0), hi = sample_code<FMT>(e[2 * k + 1], &w1);
        c.add(w0);
        c.add(w1);
        o[k] = lo | (hi << 16);
    }
    return make_uint4(o[0], o[1], o[2], o[3]);
}

// The lanes' counts -> the two counters: a reduction over the wave, the waves' sums through LDS, and one atomic per counter from
// a block whose sum is not zero (a capture on its grid issues none).
__device__ inline void add_counts(const Counts &c, unsigned long long *counters)
{
    __shared__ uint32_t wave_sum[2][4];
    uint32_t a = c.inexact, b = c.clamped;
    for (int d = warpSize / 2; d > 0; d >>= 1) {
        a += __shfl_xor(a, d);
        b += __shfl_xor(b, d);
    }
    if (counters == nullptr)
        return; // (kernel-uniform)
    const unsigned wave = threadIdx.x / warpSize;
    if (threadIdx.x % warpSize == 0) {
        wave_sum[0][wave] = a;
        wave_sum[1][wave] = b;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        const unsigned long long si = (unsigned long long)wave_sum[0][0] + wave_sum[0][1] + wave_sum[0][2] + wave_sum[0][3];
        const unsigned long long sc = (unsigned long long)wave_sum[1][0] + wave_sum[1][1] + wave_sum[1][2] + wave_sum[1][3];
        if (si)
            atomicAdd(&counters[0], si);
        if (sc)
            atomicAdd(&counters[1], sc);
    }
}

// 4 samples at p -> the two dwords of their half of a group's store
template <int FMT, class P> __device__ inline uint2 convert_half(P p, Counts &c)
{
    typename Element<FMT>::type e[4];
    __builtin_memcpy(e, p, sizeof e);
    uint32_t o[2];
    for (int k = 0; k < 2; k++) {
        uint32_t w0, w1;
        const uint32_t lo = sample_code<FMT>(e[2 * k], &w0), hi = sample_code<FMT>(e[2 * k + 1], &w1);
        c.add(w0);
        c.add(w1);
        o[k] = lo | (hi << 16);
    }
    return make_uint2(o[0], o[1]);
}

// The 64 groups of float32 samples a wave takes at once, from group `base` on: 2 KiB in, 1 KiB out.  A lane that loaded its own
// group's 32 bytes would leave every load instruction of the wave touching 2 KiB for 1 KiB of data.  Instead the wave reads the
// 2 KiB as two runs of 64 consecutive 16-byte pieces, lane L piece L and piece 64 + L: half L & 1 of group L / 2 and of group
// 32 + L / 2.  The lanes of a pair then swap one converted half each, and lane 2 j stores group j, lane 2 j + 1 group 32 + j.
// Returns the group this lane stores; *at = its number.
template <int FMT, class P> __device__ inline uint4 convert_wave_of_groups(P s, size_t base, Counts &c, size_t *at)
{
    const unsigned lane = threadIdx.x % warpSize;
    const uint2 a = convert_half<FMT>(s + 8 * base + 4 * lane, c), b = convert_half<FMT>(s + 8 * base + 4 * (64 + lane), c);
    const bool odd = lane & 1;
    const uint2 give = odd ? a : b; // the half the other lane of the pair stores
    const uint2 got = make_uint2(__shfl_xor(give.x, 1), __shfl_xor(give.y, 1));
    *at = base + (odd ? 32 : 0) + lane / 2;
    return odd ? make_uint4(got.x, got.y, b.x, b.y) : make_uint4(a.x, a.y, got.x, got.y);
}

// COUNT = false (no counters were given): the samples are not classified at all.
template <int FMT, bool COUNT>
__global__ __launch_bounds__(256) void convert_kernel(uint16_t *__restrict__ dst, const typename Element<FMT>::type *__restrict__ src,
                                                      size_t n, size_t head, unsigned long long *counters)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x, t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t groups = (n - head) / 8, tail_at = head + 8 * groups;
    Counts c;
    if (t < head) // (head <= 7, and <= n)
        dst[t] = convert_one<FMT>(src + t, c);
    if (tail_at + t < n)
        dst[tail_at + t] = convert_one<FMT>(src + tail_at + t, c);
    uint4 *d4 = reinterpret_cast<uint4 *>(dst + head); // 16-byte aligned: what head is for
    const typename Element<FMT>::type *s = src + head;
    for (size_t i = t; i - threadIdx.x % warpSize < groups; i += stride) { // (wave-uniform: the wave's first group exists)
        const size_t base = i - threadIdx.x % warpSize;                    // a multiple of 64: the block and the stride are
        size_t at = i;
        uint4 out;
        if (sizeof(typename Element<FMT>::type) == 4 && base + 64 <= groups) // (the float32 formats, real and IQ)
            out = convert_wave_of_groups<FMT>(s, base, c, &at);
        else if (i < groups)
            out = convert_group<FMT>(s + 8 * i, c);
        else
            continue;
        d4[at] = out; // (one store for both roads: 16 bytes, whole)
    }
    if (COUNT)
        add_counts(c, counters);
}

// A block takes chunks of 256 consecutive groups, grid-stride, and finds their captures as unpack12_batch.hip does: the rows of
// the chunk's first and last group by the block (block-uniform: scalar loads), a lane's own row between those two only.
template <int FMT>
__global__ __launch_bounds__(256) void convert_batch_kernel(uint16_t *__restrict__ dst, const ConvertSeg *__restrict__ tab, uint32_t n_rows,
                                                            uint64_t groups, unsigned long long *counters)
{
    const uint64_t chunks = (groups + kConvertChunk - 1) / kConvertChunk;
    Counts c;
    for (uint64_t ch = blockIdx.x; ch < chunks; ch += gridDim.x) {
        const uint64_t g0 = ch * kConvertChunk, g1 = g0 + (kConvertChunk - 1) < groups ? g0 + (kConvertChunk - 1) : groups - 1;
        const uint32_t r0 = convert_row(tab, 0, n_rows - 1, g0);
        const uint32_t r1 = convert_row(tab, r0, n_rows - 1, g1);
        const uint64_t g = g0 + threadIdx.x;
        if (g > g1)
            continue;
        const uint32_t r = convert_row(tab, r0, r1, g);
        const uint64_t k = g - tab[r].g_first, n = tab[r].n; // the group's number inside its capture; 8 k < n
        // (an address read from a table is a generic one to the compiler: said to be global memory, the loads are global_loads)
        const typename GlobalElement<FMT>::type s = (typename GlobalElement<FMT>::type)tab[r].src + 8 * k;
        uint16_t *o = dst + 8 * (tab[r].dst16 + k);
        if (8 * k + 8 <= n) {
            *reinterpret_cast<uint4 *>(o) = convert_group<FMT>(s, c);
        } else {
            for (uint64_t j = 0; 8 * k + j < n; j++)
                o[j] = convert_one<FMT>(s + j, c);
        }
    }
    add_counts(c, counters);
}

// as launch_unpack12: 8 blocks of 256 lanes per CU at most (2048 on the 256 CUs of an MI355X) stream HBM
inline unsigned blocks_for(uint64_t lanes) { return (unsigned)std::min<uint64_t>(2048, std::max<uint64_t>(1, (lanes + 255) / 256)); }

} // namespace

hipError_t launch_convert(int fmt, uint16_t *dst, const void *src, size_t n, unsigned long long *counters, hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    const size_t head = std::min<size_t>(n, ((16 - (uintptr_t)dst % 16) % 16) / sizeof(uint16_t));
    const unsigned blocks = blocks_for(std::max<size_t>((n - head) / 8, 8)); // (head and tail: the first 7 lanes of the grid)
    const uint16_t *s16 = static_cast<const uint16_t *>(src);
    const uint32_t *f32 = static_cast<const uint32_t *>(src);
    if (fmt == kFmtInt16Real && counters)
        hipLaunchKernelGGL((convert_kernel<kFmtInt16Real, true>), dim3(blocks), dim3(256), 0, stream, dst, s16, n, head, counters);
    else if (fmt == kFmtInt16Real)
        hipLaunchKernelGGL((convert_kernel<kFmtInt16Real, false>), dim3(blocks), dim3(256), 0, stream, dst, s16, n, head, counters);
    else if (fmt == kFmtFloat32Real && counters)
        hipLaunchKernelGGL((convert_kernel<kFmtFloat32Real, true>), dim3(blocks), dim3(256), 0, stream, dst, f32, n, head, counters);
    else if (fmt == kFmtFloat32Real)
        hipLaunchKernelGGL((convert_kernel<kFmtFloat32Real, false>), dim3(blocks), dim3(256), 0, stream, dst, f32, n, head, counters);
    else if (fmt == kConvFloat32Iq && counters)
        hipLaunchKernelGGL((convert_kernel<kConvFloat32Iq, true>), dim3(blocks), dim3(256), 0, stream, dst, f32, n, head, counters);
    else if (fmt == kConvFloat32Iq)
        hipLaunchKernelGGL((convert_kernel<kConvFloat32Iq, false>), dim3(blocks), dim3(256), 0, stream, dst, f32, n, head, counters);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

hipError_t launch_convert_batch(int fmt, uint16_t *dst, const ConvertSeg *tab_device, uint32_t n_rows, uint64_t groups,
                                unsigned long long *counters, hipStream_t stream)
{
    if (groups == 0 || n_rows == 0)
        return hipSuccess;
    const unsigned blocks = (unsigned)std::min<uint64_t>(2048, (groups + kConvertChunk - 1) / kConvertChunk);
    if (fmt == kFmtInt16Real)
        hipLaunchKernelGGL(convert_batch_kernel<kFmtInt16Real>, dim3(blocks), dim3(kConvertChunk), 0, stream, dst, tab_device, n_rows, groups, counters);
    else if (fmt == kFmtFloat32Real)
        hipLaunchKernelGGL(convert_batch_kernel<kFmtFloat32Real>, dim3(blocks), dim3(kConvertChunk), 0, stream, dst, tab_device, n_rows, groups, counters);
    else if (fmt == kConvFloat32Iq)
        hipLaunchKernelGGL(convert_batch_kernel<kConvFloat32Iq>, dim3(blocks), dim3(kConvertChunk), 0, stream, dst, tab_device, n_rows, groups, counters);
    else
        return hipErrorInvalidValue;
    return hipGetLastError();
}

} // namespace adsb
