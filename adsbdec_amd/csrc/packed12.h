// packed12.h -- one group of Airspy packed 12-bit samples (include/adsbdec_amd.h: the format) as ordinary uint16 samples.
// Host + device code (the one HIP type is behind __HIPCC__): the unpack kernel (unpack12.hip) and a CPU test (tests/cpp/packed12.cpp, against
// the known answers of the format) compile the same function.
//
// A group is 8 samples s0..s7 in three little-endian 32-bit words w0, w1, w2.  Read as ONE 96-bit big-endian number
// w0:w1:w2 the group is s0 s1 ... s7, 12 bits each, most significant first; two samples (s2, s5) straddle a word boundary.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "scan_kernel_format.h" // ADSB_HD

namespace adsb {

constexpr int kPackedGroupSamples = 8;
constexpr int kPackedGroupBytes = 12;

// s[k] = sample k of the group whose words are w0, w1, w2 (codes 0..4095: every uint16 has its top four bits clear)
ADSB_HD inline void unpack12_group(uint32_t w0, uint32_t w1, uint32_t w2, uint16_t s[8])
{
    s[0] = (uint16_t)(w0 >> 20);
    s[1] = (uint16_t)((w0 >> 8) & 0xfffu);
    s[2] = (uint16_t)(((w0 & 0xffu) << 4) | (w1 >> 28));
    s[3] = (uint16_t)((w1 >> 16) & 0xfffu);
    s[4] = (uint16_t)((w1 >> 4) & 0xfffu);
    s[5] = (uint16_t)(((w1 & 0xfu) << 8) | (w2 >> 24));
    s[6] = (uint16_t)((w2 >> 12) & 0xfffu);
    s[7] = (uint16_t)(w2 & 0xfffu);
}

// The same group as four dwords, samples 2k (low half) and 2k+1 (high half) in dword k: the 16-byte store of the kernel.
ADSB_HD inline void unpack12_group_pairs(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t out[4])
{
    uint16_t s[8];
    unpack12_group(w0, w1, w2, s);
    for (int k = 0; k < 4; k++)
        out[k] = (uint32_t)s[2 * k] | ((uint32_t)s[2 * k + 1] << 16);
}

#ifdef __HIPCC__
// unpack12.hip: `groups` groups at src (4-byte aligned) -> 8 * groups samples at dst (16-byte aligned), enqueued on `stream`
hipError_t launch_unpack12(uint16_t *dst, const void *src, size_t groups, hipStream_t stream);
#endif

} // namespace adsb
