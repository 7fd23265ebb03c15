// convert_rows.cpp -- the row look-up of convert_batch_kernel (csrc/sample_format.h convert_row, ConvertSeg) on the CPU: for
// tables that hold captures of 1 .. 7 samples (one short group) and of 2^29 groups side by side, the chunk-wise look-up the kernel
// does (the rows of a chunk's first and last group, then a lane's row between them) finds, for every group looked at, the row a
// plain scan of the table finds; the group's number k inside its capture has 8 k < n; and the group is short (8 k + 8 > n: the
// sample-by-sample road) only where it is its capture's last one.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../adsbdec_amd/csrc/sample_format.h"
#include "../../adsbdec_amd/csrc/stage_layout.hpp"

using adsb::ConvertSeg;

static uint64_t checked = 0, short_groups = 0;

// the last row whose first group is <= g, by a scan from row `from` on (a row at or before the answer)
static uint32_t scan_row(const std::vector<ConvertSeg> &tab, uint32_t from, uint64_t g)
{
    uint32_t r = from;
    while (r + 2 < tab.size() && tab[r + 1].g_first <= g)
        r++;
    return r;
}

// want: the row a plain scan of the table finds for g
static bool check_group(const std::vector<ConvertSeg> &tab, uint64_t g, uint32_t want)
{
    const uint32_t n_rows = (uint32_t)tab.size() - 1;
    const uint64_t groups = tab[n_rows].g_first, chunk = adsb::kConvertChunk;
    // the kernel's three steps
    const uint64_t g0 = g / chunk * chunk, g1 = g0 + (chunk - 1) < groups ? g0 + (chunk - 1) : groups - 1;
    const uint32_t r0 = adsb::convert_row(tab.data(), 0, n_rows - 1, g0);
    const uint32_t r1 = adsb::convert_row(tab.data(), r0, n_rows - 1, g1);
    const uint32_t r = adsb::convert_row(tab.data(), r0, r1, g);
    checked++;
    if (r != want || r >= n_rows || g >= tab[r + 1].g_first) {
        printf("group %llu: row %u, a scan finds %u of %u (chunk rows %u .. %u)\n", (unsigned long long)g, r, want, n_rows, r0, r1);
        return false;
    }
    const uint64_t k = g - tab[r].g_first, n = tab[r].n;
    const bool last = g + 1 == tab[r + 1].g_first;
    if (!(8 * k < n) || ((8 * k + 8 > n) && !last)) {
        printf("group %llu: row %u, k = %llu, n = %llu, last = %d\n", (unsigned long long)g, r, (unsigned long long)k, (unsigned long long)n, (int)last);
        return false;
    }
    short_groups += 8 * k + 8 > n;
    return true;
}

int main()
{
    std::mt19937_64 rng(20261019);
    int tables = 0;
    for (int t = 0; t < 200; t++) {
        // captures of 1 .. 7 samples, of a few groups, of about a chunk, of many chunks, and now and then one of 2^29 groups (the
        // last of them short or not)
        std::vector<uint64_t> len; // samples
        const int n = 1 + (int)(rng() % 300);
        for (int i = 0; i < n; i++) {
            const unsigned kind = (unsigned)(rng() % 16);
            len.push_back(kind < 5    ? 1 + rng() % 7
                          : kind < 7  ? 1 + rng() % 40
                          : kind < 10 ? 8 * (250 + rng() % 12) - rng() % 8
                          : kind < 15 ? 1 + rng() % 1600000
                                      : 8 * (1ull << 29) - rng() % 16);
        }
        if (t == 0)
            len = {1, 8ull << 29, 7, 3, (8ull << 29) - 7, 8 * 255, 1, 8 * 256 - 1, 8 * 257, 8 * 255 + 1, 2};
        if (t == 1) { // more than a chunk of one-group captures in a row
            len.clear();
            for (int i = 0; i < 700; i++)
                len.push_back(1 + rng() % 7);
        }
        // the table as the product builds it (convert_table over stage_layout's offsets: decoder_stage.hip)
        std::vector<size_t> ns(len.begin(), len.end()), bytes, off(len.size());
        for (size_t l : ns)
            bytes.push_back(l * sizeof(uint16_t));
        adsb::stage_layout(len.size(), bytes.data(), 128, off.data());
        const std::vector<const void *> src(len.size(), nullptr);
        std::vector<ConvertSeg> tab(len.size() + 1);
        uint64_t g = 0;
        if (adsb::convert_table(len.size(), src.data(), ns.data(), off.data(), tab.data(), &g) != len.size())
            return 1;
        tables++;
        // every group within a chunk and a half of every capture boundary, in rising order (each once: the windows of short
        // captures overlap), so that ONE scan of the table, which only ever moves forward, names every group's row; and random ones
        uint64_t next = 0; // the first group not looked at yet
        uint32_t row = 0;
        for (size_t r = 0; r + 1 < tab.size(); r++) {
            const uint64_t lo = tab[r].g_first > 384 ? tab[r].g_first - 384 : 0, hi = std::min<uint64_t>(g, tab[r].g_first + 385);
            for (uint64_t at = std::max(lo, next); at < hi; at++) {
                row = scan_row(tab, row, at);
                if (!check_group(tab, at, row))
                    return 1;
            }
            next = std::max(next, hi);
        }
        for (int k = 0; k < 2000; k++) {
            const uint64_t at = k == 0 ? 0 : k == 1 ? g - 1 : rng() % g;
            if (!check_group(tab, at, scan_row(tab, 0, at)))
                return 1;
        }
    }
    if (short_groups < 20000) { // (some 150 rows a table, most of them with a short last group, each looked at once)
        printf("only %llu short groups looked up\n", (unsigned long long)short_groups);
        return 1;
    }
    printf("ok: %d tables, %llu groups looked up, %llu of them short\n", tables, (unsigned long long)checked, (unsigned long long)short_groups);
    return 0;
}
