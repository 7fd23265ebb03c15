// unpack12_rows.cpp -- the row look-up of unpack12_batch_kernel (csrc/packed12.h unpack12_row) on the CPU: for tables that hold
// captures of 1 group and of 2^29 groups side by side, the chunk-wise look-up the kernel does (the rows of a chunk's first and
// last group, then a lane's row between them) finds, for every group looked at, the row a plain scan of the table finds.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../adsbdec_amd/csrc/packed12.h"
#include "../../adsbdec_amd/csrc/stage_layout.hpp"

using adsb::Unpack12Seg;

static uint64_t checked = 0;

static bool check_group(const std::vector<Unpack12Seg> &tab, uint64_t g)
{
    const uint32_t n_rows = (uint32_t)tab.size() - 1;
    const uint64_t groups = tab[n_rows].g_first, chunk = adsb::kUnpack12Chunk;
    const uint64_t g0 = g / chunk * chunk, g1 = g0 + chunk - 1 < groups ? g0 + chunk - 1 : groups - 1;
    const uint32_t r0 = adsb::unpack12_row(tab.data(), 0, n_rows - 1, g0);
    const uint32_t r1 = adsb::unpack12_row(tab.data(), r0, n_rows - 1, g1);
    const uint32_t r = adsb::unpack12_row(tab.data(), r0, r1, g);
    checked++;
    if (r >= n_rows || tab[r].g_first > g || g >= tab[r + 1].g_first) {
        printf("group %llu: row %u of %u (chunk rows %u .. %u)\n", (unsigned long long)g, r, n_rows, r0, r1);
        return false;
    }
    return true;
}

int main()
{
    std::mt19937_64 rng(20261017);
    int tables = 0;
    for (int t = 0; t < 200; t++) {
        // captures of 1 .. a few groups, of about a chunk, of many chunks, and now and then one of 2^29 groups
        std::vector<uint64_t> len;
        const int n = 1 + (int)(rng() % 300);
        for (int i = 0; i < n; i++) {
            const unsigned kind = (unsigned)(rng() % 16);
            len.push_back(kind < 6 ? 1 + rng() % 3 : kind < 10 ? 250 + rng() % 12 : kind < 15 ? 1 + rng() % 200000 : (1ull << 29) - (rng() % 2));
        }
        if (t == 0)
            len = {1, 1ull << 29, 1, 1, (1ull << 29) - 1, 255, 1, 256, 257};
        // the table as the product builds it (unpack12_table over stage_layout's offsets: decoder_stage.hip)
        std::vector<size_t> ns, bytes, off(len.size());
        for (uint64_t l : len) {
            ns.push_back((size_t)l * adsb::kPackedGroupSamples);
            bytes.push_back(ns.back() * sizeof(uint16_t));
        }
        adsb::stage_layout(len.size(), bytes.data(), 128, off.data());
        const std::vector<const void *> src(len.size(), nullptr);
        std::vector<Unpack12Seg> tab(len.size() + 1);
        uint64_t g = 0;
        if (adsb::unpack12_table(len.size(), src.data(), ns.data(), off.data(), tab.data(), &g) != len.size())
            return 1;
        tables++;
        // every group within a chunk and a half of every capture boundary, and random ones
        for (size_t r = 0; r + 1 < tab.size(); r++)
            for (int64_t d = -384; d <= 384; d++) {
                const int64_t at = (int64_t)tab[r].g_first + d;
                if (at >= 0 && (uint64_t)at < g && !check_group(tab, (uint64_t)at))
                    return 1;
            }
        for (int k = 0; k < 2000; k++)
            if (!check_group(tab, rng() % g))
                return 1;
        if (!check_group(tab, g - 1) || !check_group(tab, 0))
            return 1;
    }
    printf("ok: %d tables, %llu groups looked up\n", tables, (unsigned long long)checked);
    return 0;
}
