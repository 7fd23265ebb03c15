// level_tail.h -- the reduction tail of the level report, device code shared by level_kernel.hip (one capture) and
// level_batch_kernel.hip (a batch of captures): the wave-uniform counters, a run's 28 bit patterns into a histogram in LDS and
// one unsigned maximum, and the rail counters of the codes a lane owns.  Moved here from level_kernel.hip word for word when
// the batch unit came: everything is forced inline in an anonymous namespace, and level_kernel.hip compiles to the
// instructions it had with these lines of its own (profiles/r26_level_batch_isa_identity.txt).
// Included behind scan_stages.h (kRun, f32x2, iq_power, iq8_power) and level.h (kLevelIq16 ..).
#pragma once

#ifndef ADSB_LEVEL_HIST
#define ADSB_LEVEL_HIST 5
#endif

namespace adsb {

namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));

// lanes of the wave for which p holds (wave-uniform: the scalar side counts)
__device__ __forceinline__ uint32_t lanes(bool p) { return (uint32_t)__builtin_popcountll(__ballot(p)); }

struct Counts { // wave-uniform, over the wave's passes
    uint32_t negative = 0, rail_lo = 0, rail_hi = 0, over = 0;
};

// one increment per lane with `on`
__device__ __forceinline__ void hist_add(uint32_t *hist, const uint32_t bin, const bool on, const int lane)
{
#if ADSB_LEVEL_HIST & 2
    const unsigned long long act = __ballot(on);
    if (act == 0)
        return;
    const int first = __builtin_ctzll(act);
    const uint32_t b0 = (uint32_t)__builtin_amdgcn_readlane((int)bin, first);
    if (__ballot(on && bin == b0) == act) { // (wave-uniform)
        if (lane == first)
            atomicAdd(&hist[b0], (uint32_t)__builtin_popcountll(act));
        return;
    }
#endif
    if (on)
        atomicAdd(&hist[bin], 1u);
}

// The reduction tail of one run: b[k] is the bit pattern of the lane's power sample k, of which the first `left` exist (kFull: all
// 28, in every lane of the wave).  kSigned: a sample may have its sign bit set (never behind a front end that squares and adds).
// Returns the run's envelope bits.
template <bool kFull, bool kSigned>
__device__ __forceinline__ uint32_t level_tail(const uint32_t (&b)[kRun], const int left, uint32_t *hist, Counts &c, const int lane)
{
    uint32_t mx = 0;
#if ADSB_LEVEL_HIST & 4
    uint32_t mn = 0xFFFFFFFFu, n_on = (kFull && !kSigned) ? kRun : 0;
#endif
#pragma unroll
    for (int k = 0; k < kRun; k++) {
        const bool have = kFull || k < left;
        const bool minus = kSigned && (int32_t)b[k] < 0;
        if (kSigned)
            c.negative += lanes(have && minus);
        const bool on = have && !minus;
        mx = max(mx, on ? b[k] : 0u);
#if ADSB_LEVEL_HIST & 4
        mn = min(mn, on ? b[k] : 0xFFFFFFFFu);
        if (!(kFull && !kSigned))
            n_on += on;
#else
        hist_add(hist, b[k] >> 20, on, lane);
#endif
    }
#if ADSB_LEVEL_HIST & 4
    // the run-uniform shortcut: smallest and largest counted pattern in one bin (no counted sample: 4095 against 0) -> one add
    if ((mn >> 20) == (mx >> 20)) {
        atomicAdd(&hist[mx >> 20], n_on);
    } else {
#pragma unroll
        for (int k = 0; k < kRun; k++)
            if ((kFull || k < left) && !(kSigned && (int32_t)b[k] < 0))
                atomicAdd(&hist[b[k] >> 20], 1u);
    }
#endif
    return mx;
}

// The codes of the pairs a lane owns (slots 6 .. 33 of its window) as the typed loads hand them over -- integers 0 .. 65535, exact
// in binary32 -- on the ADC's rails and beyond them.  First the lane's smallest and largest code (as bit patterns: floats that are
// not negative order as their words do); a pass in which no lane has a 0 or a code from 4095 up -- most passes of most captures --
// counts nothing.
template <bool kFull> __device__ __forceinline__ void rails_real(const f32x2 (&vv)[34], const int left, Counts &c)
{
    uint32_t lo = 0xFFFFFFFFu, hi = 0;
#pragma unroll
    for (int k = 0; k < kRun; k++) {
        const float fx = vv[6 + k].x, fy = vv[6 + k].y; // (copies: a bit cast of the vector's element itself reads element 0 for both)
        const uint32_t x = __builtin_bit_cast(uint32_t, fx), y = __builtin_bit_cast(uint32_t, fy);
        lo = min(min(lo, x), y); // (a ragged run's codes behind `left` too: they can only send the pass to the counting below)
        hi = max(max(hi, x), y);
    }
    if (__ballot(lo == 0u || hi >= __builtin_bit_cast(uint32_t, 4095.0f)) == 0) // (wave-uniform)
        return;
#pragma unroll
    for (int k = 0; k < kRun; k++) {
        const bool have = kFull || k < left;
        const f32x2 v = vv[6 + k];
        c.rail_lo += lanes(have && v.x == 0.0f) + lanes(have && v.y == 0.0f);
        c.rail_hi += lanes(have && v.x == 4095.0f) + lanes(have && v.y == 4095.0f);
        c.over += lanes(have && v.x > 4095.0f) + lanes(have && v.y > 4095.0f);
    }
}

// ... of complex samples: u[k] = (I, Q) as two int16 (kKind == kLevelIq16) or two int8 in the low half (kLevelIq8), on the format's
// minimum and maximum.  The same pre-check with packed 16-bit minima and maxima (int8: of the widened twin, I << 8 and Q << 8).
typedef short s16x2 __attribute__((ext_vector_type(2)));
template <int kKind, bool kFull> __device__ __forceinline__ void rails_iq(const uint32_t (&u)[kRun], const int left, Counts &c)
{
    constexpr uint32_t kMask = kKind == kLevelIq8 ? 0xFFu : 0xFFFFu, kLo = kKind == kLevelIq8 ? 0x80u : 0x8000u, kHi = kLo - 1;
    constexpr int kShift = kKind == kLevelIq8 ? 8 : 16;
    s16x2 lo = {32767, 32767}, hi = {-32768, -32768};
#pragma unroll
    for (int k = 0; k < kRun; k++) {
        const uint32_t w = kKind == kLevelIq8 ? __builtin_amdgcn_perm(0u, u[k], 0x010C000Cu) : u[k]; // bytes (0, I, 0, Q)
        const s16x2 v = __builtin_bit_cast(s16x2, w);
        lo = __builtin_elementwise_min(lo, v);
        hi = __builtin_elementwise_max(hi, v);
    }
    constexpr short kTop = kKind == kLevelIq8 ? 0x7F00 : 0x7FFF;
    if (__ballot(lo.x == -32768 || lo.y == -32768 || hi.x == kTop || hi.y == kTop) == 0) // (wave-uniform)
        return;
#pragma unroll
    for (int k = 0; k < kRun; k++) {
        const bool have = kFull || k < left;
        const uint32_t i = u[k] & kMask, q = (u[k] >> kShift) & kMask;
        c.rail_lo += lanes(have && i == kLo) + lanes(have && q == kLo);
        c.rail_hi += lanes(have && i == kHi) + lanes(have && q == kHi);
    }
}

// The bit pattern of unit u's power sample, and its scalars on the rails: int16 -32768 / 32767, int8 -128 / 127.
template <int kKind> __device__ __forceinline__ uint32_t unit_bits(const uint32_t u)
{
    return kKind == kLevelIq16 ? __builtin_bit_cast(uint32_t, iq_power(u)) : kKind == kLevelIq8 ? __builtin_bit_cast(uint32_t, iq8_power(u)) : u;
}

} // namespace

} // namespace adsb
