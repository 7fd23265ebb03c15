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

// The inverse: the words of the group whose samples are s[0..7], each taken & 0xfff (gather_pack12_kernel.hip packs a capture's
// bursts with it; tests/cpp/pack12_group.cpp holds it to unpack12_group and to the known answers of the format).
ADSB_HD inline void pack12_group(const uint16_t s[8], uint32_t w[3])
{
    uint32_t c[8];
    for (int k = 0; k < 8; k++)
        c[k] = s[k] & 0xfffu;
    w[0] = (c[0] << 20) | (c[1] << 8) | (c[2] >> 4);
    w[1] = ((c[2] & 0xfu) << 28) | (c[3] << 16) | (c[4] << 4) | (c[5] >> 8);
    w[2] = ((c[5] & 0xffu) << 24) | (c[6] << 12) | c[7];
}

// The same group as four dwords, samples 2k (low half) and 2k+1 (high half) in dword k: the 16-byte store of the kernel.
ADSB_HD inline void unpack12_group_pairs(uint32_t w0, uint32_t w1, uint32_t w2, uint32_t out[4])
{
    uint16_t s[8];
    unpack12_group(w0, w1, w2, s);
    for (int k = 0; k < 4; k++)
        out[k] = (uint32_t)s[2 * k] | ((uint32_t)s[2 * k + 1] << 16);
}

// unpack12_batch.hip: the captures of a batch in one launch.  A row per capture that has groups, in capture order: its groups
// are numbered g_first .. (the next row's g_first - 1), read from src (4-byte aligned) and written from dst + 8 * dst16 on (dst16
// counts 16-byte units; dst itself 16-byte aligned).  Row n_rows, behind the last one, holds the number of all groups.
struct Unpack12Seg {
    uint64_t src;
    uint64_t dst16;
    uint64_t g_first;
};
constexpr unsigned kUnpack12Chunk = 256; // consecutive groups a block looks its rows up for at once (= its lanes)

// The last row of tab[lo .. hi] whose first group is <= g (tab[lo].g_first <= g is the caller's): the kernel's look-up, for a
// chunk's first and last group by the block and between those two rows by a lane (tests/cpp/unpack12_rows.cpp runs it on the CPU).
ADSB_HD inline uint32_t unpack12_row(const Unpack12Seg *tab, uint32_t lo, uint32_t hi, uint64_t g)
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
// The table of n_captures packed captures into tab[0 .. rows], rows <= n_captures: capture i has n[i] samples (whole groups), is
// read at src[i] and written off[i] bytes (a multiple of 16) into the launch's dst.  *groups = the number of all groups.  Returns the
// rows, the closing one not counted.
inline uint32_t unpack12_table(size_t n_captures, const void *const *src, const size_t *n, const size_t *off, Unpack12Seg *tab, uint64_t *groups)
{
    uint32_t row = 0;
    uint64_t at = 0;
    for (size_t i = 0; i < n_captures; i++) {
        if (n[i] == 0)
            continue;
        tab[row++] = Unpack12Seg{(uint64_t)(uintptr_t)src[i], off[i] / 16, at};
        at += n[i] / kPackedGroupSamples;
    }
    tab[row] = Unpack12Seg{0, 0, at}; // behind the last row: where its groups end
    *groups = at;
    return row;
}

#ifdef __HIPCC__
// unpack12.hip: `groups` groups at src (4-byte aligned) -> 8 * groups samples at dst (16-byte aligned), enqueued on `stream`
hipError_t launch_unpack12(uint16_t *dst, const void *src, size_t groups, hipStream_t stream);

hipError_t launch_unpack12_batch(uint16_t *dst, const Unpack12Seg *tab_device, uint32_t n_rows, uint64_t groups, hipStream_t stream);
#endif

} // namespace adsb
