// power_ordered.h -- device code that the scan kernel (scan_kernel.hip: pw_at, stage_b) and the seam kernel (seam_kernel.hip)
// both use: the FIR taps, a power sample at a run-time index in the reference's summation order, and the transpose of a
// sliced frame's column bytes.  One definition, so that the two kernels cannot round differently.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace adsb {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

namespace {

// air.c:36-45. Each tap is (float)<double literal>, as in the reference's
// `static const float dsfilter[] = { 0.012627, ... }`.
template <int K>
__device__ __forceinline__ constexpr float tap()
{
    constexpr double lit[14] = {0.012627, 0.025254, 0.037881, 0.050508, 0.063135,
                                0.075761, 0.088388, 0.088388, 0.075761, 0.063135,
                                0.050508, 0.037881, 0.025254, 0.012627};
    return (float)lit[K];
}

// Same arithmetic for power samples at RUN-TIME indices (rare path: pw of a
// CRC-valid candidate needs a[g], a[g+10], a[g+35], a[g+45]).  Rounds exactly like
// power_sample<>: same products, same order (one static order per phase p = m mod
// 7), first product not added to zero.  All loads are issued before any use: the
// whole workgroup waits for this path at the next barrier.
template <int P>
__device__ __forceinline__ float power_ordered(const f32x2 (&pr)[7])
{
    // pr[a] = (T[12-2a], T[13-2a]) * (I, Q) of the pair of age a; order p, p-1, .., 0, 6, .., p+1
    f32x2 s = pr[P];
#pragma unroll
    for (int a = P - 1; a >= 0; a--)
        s = s + pr[a];
#pragma unroll
    for (int a = 6; a > P; a--)
        s = s + pr[a];
    const f32x2 sq = s * s;
    return sq.x + sq.y;
}

// power_ordered<p> with p = m mod 7 chosen at run time
__device__ __forceinline__ float power_by_phase(const f32x2 (&pr)[7], int p)
{
    float r;
    switch (p) {
    case 0: r = power_ordered<0>(pr); break;
    case 1: r = power_ordered<1>(pr); break;
    case 2: r = power_ordered<2>(pr); break;
    case 3: r = power_ordered<3>(pr); break;
    case 4: r = power_ordered<4>(pr); break;
    case 5: r = power_ordered<5>(pr); break;
    default: r = power_ordered<6>(pr); break;
    }
    return r;
}

// The slicer gathers the frame as 14 column bytes (frame bit k = 14 b + c is bit b
// of column c; four columns per word).  Rebuild the 14 frame bytes in order (bit k
// is bit 7 - k%8 of byte k/8), packed little-endian into wds[0..3], with the
// length in byte 14.  A static 112-bit transpose: 2 operations per bit.
__device__ __forceinline__ void columns_to_bytes(const uint32_t (&cw)[4], bool is_short, uint32_t (&wds)[4])
{
    wds[0] = wds[1] = wds[2] = wds[3] = 0;
#pragma unroll
    for (int k = 0; k < 112; k++) {
        const int b = k / 14, c = k % 14;
        const uint32_t bit = (cw[c >> 2] >> (8 * (c & 3) + b)) & 1u;
        const int n = k >> 3;
        wds[n >> 2] |= bit << (8 * (n & 3) + 7 - (k & 7));
    }
    if (is_short) { // DF11: 56 bits = 7 bytes
        wds[1] &= 0x00FFFFFFu;
        wds[2] = 0;
        wds[3] = 0;
    }
    wds[3] |= (is_short ? 7u : 14u) << 16;
}

} // namespace
} // namespace adsb
