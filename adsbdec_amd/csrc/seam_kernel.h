// seam_kernel.h -- launch interface of the seam kernel (seam_kernel.hip): the offsets around a wrap of the reference's 32-bit
// sample counter (air.c:34), which the scan kernel's launches leave out (DESIGN.md "Input domain").
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace adsb {

// A power index is g = w * 2^31 + r: epoch w starts at power sample P = w * kEpoch (input sample w * 2^32).
constexpr uint64_t kEpoch = 1ull << 31;
constexpr int kSeamWindow = 1196;   // ADSB_WINDOW: offsets from P - 1196 on read a transient sample (P - 1 .. P + 5)
constexpr int kSeamBehind = 28;     // ... up to P + 5; the scan kernel's first launch of the epoch starts at its run boundary r = 28
constexpr int kSeamMaxOffsets = kSeamWindow + kSeamBehind;
constexpr int kSeamOutHeader = 8;   // words in front of the records: [0] records, [1] try words
// Seam offsets of the wrap at P are [P - kSeamWindow, P + kSeamBehind).
inline uint64_t seam_first(uint64_t P) { return P - kSeamWindow; }
inline uint64_t seam_end(uint64_t P) { return P + kSeamBehind; }

struct SeamArgs {
    const uint32_t *x;     // (I,Q) pairs; x[0] is ABSOLUTE stream pair index pbuf0
    int64_t pbuf0;
    int64_t p_lo, p_hi;    // absolute pair indices present in the buffer; others read as silence
    uint64_t boundary;     // P = w * kEpoch, w >= 1
    uint64_t g_begin;      // absolute offsets [g_begin, g_end) inside [seam_first(P), seam_end(P))
    uint64_t g_end;
    int df18;
    const uint32_t *synd;    // ScanArgs::synd
    const uint32_t *fix_tab; // ScanArgs::fix_tab, or null
    uint32_t fix_mul;
    int want_tries;
    // out[0] = n records, out[1] = n try words; records {g - g_begin, pw, frame | len << 16 | flags << 24} (kCandWords each) from
    // out + kSeamOutHeader, try words ((g - g_begin) << 2) | code from out + kSeamOutHeader + kCandWords * kSeamMaxOffsets.
    // Neither list is sorted.  Every CRC-valid offset is reported (no never-visited filter).
    uint32_t *out;
    // diagnostics (adsb_seam_power): null in every launch a stream makes.  Set: the launch's n_pow = g_end - g_begin - 1 + kSeamWindow
    // power samples, power_out[i] = power sample g_begin + i, as the offsets' tests read them.
    float *power_out;
};
constexpr size_t kSeamOutWords = kSeamOutHeader + (6 + 1) * (size_t)kSeamMaxOffsets;

hipError_t launch_seam(const SeamArgs &args, hipStream_t stream);

} // namespace adsb
