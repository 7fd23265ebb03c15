// sample_format.h -- one sample of the two real formats beside the uint16 code (include/adsbdec_amd.h: the formats) as that code.
// Host + device code (the HIP types are behind __HIPCC__): the conversion kernels (convert_samples.hip) and a CPU test
// (tests/cpp/sample_formats.cpp, every int16 value and the float edge cases against the definition) compile the same functions.
//
// Written from the formats' definitions as airspy_rx -t names them, not checked against libairspy (it is not at hand):
//   INT16_REAL    x = (code - 2048) << 4, little-endian int16.   code = (x >> 4) + 2048 (arithmetic shift): total, always in
//                 [0, 4095].  Inexact iff x & 15 != 0.
//   FLOAT32_REAL  x = (code - 2048) / 2048, binary32 (exact).     r = rint(2048 x), ties to even; code = r + 2048 clamped to
//                 [0, 4095].  Clamped iff r + 2048 lies outside [0, 4095] or x is +-Inf or NaN (NaN -> 2048).  Otherwise inexact iff
//                 (code - 2048) / 2048 is not the value x: -0.0 is exact, every non-zero denormal is inexact (-> 2048) -- decided
//                 on the bit pattern, so the answer is the same whatever the denormal mode of the unit that runs this.
//   FLOAT32_IQ    (the _iq calls, fmt 0) one SCALAR of a complex sample, nominal range [-1, 1): r = rint(32768 x), ties to even,
//                 clamped to [-32768, 32767] -- the int16 scalar of INT16_IQ (fmt 2), which the scan then reads.  Clamped iff r lies
//                 outside or x is +-Inf or NaN (NaN -> 0).  Otherwise inexact iff r is not 32768 x: -0.0 is exact, every non-zero
//                 denormal is inexact (-> 0), decided on the bit pattern as for FLOAT32_REAL.  A quantisation to 1/16 ADC LSB:
//                 libairspy's float path need not sit on that grid, so real fmt-0 files are expected to report inexact samples.
// A sample is counted at most once; clamped wins.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "scan_kernel_format.h" // ADSB_HD

namespace adsb {

// fmt values of the _as calls: the numbers airspy_rx -t takes
constexpr int kFmtFloat32Real = 1, kFmtInt16Real = 3, kFmtUint16Real = 4, kFmtRaw = 5;

// The library's own number for the scalars of FLOAT32_IQ where a conversion is named (launch_convert*, push_copy's conv): not an
// airspy_rx -t number -- that one is 0, which the _as calls refuse -- and no _as call accepts it (format_element_bytes: 0).
constexpr int kConvFloat32Iq = 8;

// fmt values of the _iq calls (include/adsbdec_amd.h).  kFmtInt8Iq is the PUBLIC number 8 and has nothing to do with kConvFloat32Iq,
// which happens to be 8 too: an int8 capture is never converted (scan_iq8_kernel.hip reads it as it is), so the public number
// never reaches a conversion -- the _iq calls map it to the stream kind kKindIq8 (decoder_state.hpp) at the boundary, conv = 0.
constexpr int kFmtFloat32Iq = 0, kFmtInt16Iq = 2, kFmtInt8Iq = 8;

// bytes of one complex sample of an _iq format (0: not one)
ADSB_HD constexpr size_t iq_sample_bytes(int fmt) { return fmt == kFmtInt8Iq ? 2 : fmt == kFmtInt16Iq ? 4 : fmt == kFmtFloat32Iq ? 8 : 0; }

// The power sample of ONE int8 IQ sample d = (I, Q), two signed bytes in the low 16 bits: the INT16_IQ power sample of the widened
// twin (I << 8, Q << 8) -- i = 16 I, q = 16 Q, a = fl(fl(i i) + fl(q q)) = 256 (I^2 + Q^2), an integer of at most 2^23: every product
// and the sum are exact in binary32, so nothing here rounds and a fused form would give the same bits.
ADSB_HD inline float iq8_power(uint32_t d)
{
    const float i = (float)(16 * (int)(int8_t)(uint8_t)(d & 0xFFu)), q = (float)(16 * (int)(int8_t)(uint8_t)((d >> 8) & 0xFFu));
    return i * i + q * q;
}

constexpr uint32_t kSampleExact = 0, kSampleInexact = 1, kSampleClamped = 2;

// bytes per sample of a converted format (0: not one)
ADSB_HD constexpr size_t format_element_bytes(int fmt) { return fmt == kFmtFloat32Real ? 4 : fmt == kFmtInt16Real ? 2 : 0; }

// bytes per element of anything a conversion kernel reads: the _as formats and the scalars of FLOAT32_IQ
ADSB_HD constexpr size_t convert_element_bytes(int conv) { return conv == kConvFloat32Iq ? 4 : format_element_bytes(conv); }

// x: the 16 bits of the sample.  Returns the code; *what = kSampleExact / kSampleInexact.
ADSB_HD inline uint32_t int16_real_code(uint32_t x, uint32_t *what)
{
    *what = (x & 15u) ? kSampleInexact : kSampleExact;
    return (uint32_t)(((int32_t)(int16_t)(uint16_t)x >> 4) + 2048);
}

// bits: the 32 bits of the sample.  Returns the code; *what = kSampleExact / kSampleInexact / kSampleClamped.
ADSB_HD inline uint32_t float32_real_code(uint32_t bits, uint32_t *what)
{
    // Without a branch: eight samples a lane, and lanes that disagree would walk every path one after the other.
    const uint32_t e = (bits >> 23) & 0xffu, m = bits & 0x7fffffu;
    const bool nan = e == 0xffu && m != 0;
    float x;
    __builtin_memcpy(&x, &bits, sizeof x);
    const float y = x * 2048.0f; // exact (a power of two) for a normal x, or +-Inf; a denormal x is judged by its bits below
    const float r = rintf(y);    // ties to even (the default rounding mode; v_rndne_f32 on the device)
    const bool lo = r < -2048.0f, hi = r > 2047.0f; // (both false for NaN; +-Inf ends here)
    const float rc = nan ? 0.0f : lo ? -2048.0f : hi ? 2047.0f : r;
    // (code - 2048) / 2048 == x  <=>  r == 2048 x; e == 0: +-0.0 is the grid point 2048, and a denormal -- rint(2048 x) = 0 with or
    // without flushing -- is not 0
    const bool off = e == 0 ? m != 0 : !(r == y);
    *what = (nan || lo || hi) ? kSampleClamped : off ? kSampleInexact : kSampleExact;
    return (uint32_t)((int32_t)rc + 2048);
}

// bits: the 32 bits of one scalar of a FLOAT32_IQ sample.  Returns the int16 scalar as its 16 bits; *what as float32_real_code.
ADSB_HD inline uint32_t float32_iq_code(uint32_t bits, uint32_t *what)
{
    const uint32_t e = (bits >> 23) & 0xffu, m = bits & 0x7fffffu;
    const bool nan = e == 0xffu && m != 0;
    float x;
    __builtin_memcpy(&x, &bits, sizeof x);
    const float y = x * 32768.0f; // exact (a power of two) for a normal x, or +-Inf; a denormal x is judged by its bits below
    const float r = rintf(y);     // ties to even
    const bool lo = r < -32768.0f, hi = r > 32767.0f; // (both false for NaN; +-Inf ends here)
    const float rc = nan ? 0.0f : lo ? -32768.0f : hi ? 32767.0f : r;
    const bool off = e == 0 ? m != 0 : !(r == y); // +-0.0 is the grid point 0; a denormal rounds to 0 and is not 0
    *what = (nan || lo || hi) ? kSampleClamped : off ? kSampleInexact : kSampleExact;
    return (uint32_t)(int32_t)rc & 0xffffu;
}

template <int FMT> ADSB_HD inline uint32_t sample_code(uint32_t bits, uint32_t *what)
{
    return FMT == kFmtInt16Real ? int16_real_code(bits, what) : FMT == kConvFloat32Iq ? float32_iq_code(bits, what) : float32_real_code(bits, what);
}

// convert_samples.hip, the captures of a batch in one launch (the scheme of packed12.h's Unpack12Seg).  A capture of n samples is
// ceil(n / 8) groups of 8, the last one possibly short; the groups of all captures are numbered in one space.  A row per capture
// THAT HAS SAMPLES, in capture order: its groups are g_first .. (the next row's g_first - 1), read from src (aligned to the
// element) and written from dst + 8 * dst16 on (dst16 counts 16-byte units; dst itself 16-byte aligned).  Row n_rows, behind the
// last one, holds the number of all groups.
struct ConvertSeg {
    uint64_t src;
    uint64_t dst16;
    uint64_t g_first;
    uint64_t n;
};
constexpr unsigned kConvertChunk = 256; // consecutive groups a block looks its rows up for at once (= its lanes)

// The last row of tab[lo .. hi] whose first group is <= g (tab[lo].g_first <= g is the caller's).
ADSB_HD inline uint32_t convert_row(const ConvertSeg *tab, uint32_t lo, uint32_t hi, uint64_t g)
{
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (tab[mid].g_first <= g)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// ---- host-only: building the table ----
// The table of n_captures captures into tab[0 .. rows], rows <= n_captures: capture i has n[i] samples (its last group may be short),
// is read at src[i] and written off[i] bytes (a multiple of 16) into the launch's dst.  *groups = the number of all groups.  Returns
// the rows, the closing one not counted.
inline uint32_t convert_table(size_t n_captures, const void *const *src, const size_t *n, const size_t *off, ConvertSeg *tab, uint64_t *groups)
{
    uint32_t row = 0;
    uint64_t at = 0;
    for (size_t i = 0; i < n_captures; i++) {
        if (n[i] == 0)
            continue;
        tab[row++] = ConvertSeg{(uint64_t)(uintptr_t)src[i], off[i] / 16, at, n[i]};
        at += (n[i] + 7) / 8;
    }
    tab[row] = ConvertSeg{0, 0, at, 0}; // behind the last row: where its groups end
    *groups = at;
    return row;
}

#ifdef __HIPCC__
// n samples of format fmt (kFmtFloat32Real / kFmtInt16Real; kConvFloat32Iq: n scalars -> n int16) at src (aligned to the element) -> n uint16 codes at dst (2-byte
// aligned), enqueued on `stream`; counters: NULL, or two uint64 in device memory that the samples' inexact and clamped counts are
// ADDED to (only where they are not zero).
hipError_t launch_convert(int fmt, uint16_t *dst, const void *src, size_t n, unsigned long long *counters, hipStream_t stream);

hipError_t launch_convert_batch(int fmt, uint16_t *dst, const ConvertSeg *tab_device, uint32_t n_rows, uint64_t groups,
                                unsigned long long *counters, hipStream_t stream);
#endif

} // namespace adsb
