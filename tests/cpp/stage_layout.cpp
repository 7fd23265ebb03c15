// stage_layout.cpp -- what decoder_stage.hip lays a batch out with, on the CPU: stage_layout (csrc/stage_layout.hpp) and the tables
// of the one unpack or conversion launch (csrc/packed12.h unpack12_table, csrc/sample_format.h convert_table), against a plain
// restatement for seeded capture lists.  Lengths of 0 and 1 .. 9 samples, now and then one of 2^29 groups, empty captures first,
// last and adjacent: every offset is a multiple of the alignment, the captures do not overlap and sit in order, the total is the
// last end; a table has rows only for captures with groups, each row names its capture's source, offset and first group, and the
// closing row holds the total; the offsets adsb_batch_unpacked_copy is fed (off / 2, then total / 2) are the layout's.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../adsbdec_amd/csrc/packed12.h"
#include "../../adsbdec_amd/csrc/sample_format.h"
#include "../../adsbdec_amd/csrc/stage_layout.hpp"

using namespace adsb;

#define CHECK(c)                                                            \
    do {                                                                    \
        if (!(c)) {                                                         \
            printf("list %d: %s (line %d)\n", list_no, #c, __LINE__);       \
            return false;                                                   \
        }                                                                   \
    } while (0)

static int list_no = 0;
static uint64_t rows_seen = 0, empties_seen = 0;

static bool check_list(const std::vector<size_t> &n, bool packed)
{
    const size_t k = n.size();
    std::vector<const void *> src(k);
    for (size_t i = 0; i < k; i++)
        src[i] = reinterpret_cast<const void *>((uintptr_t)0x1000 * (i + 1));
    for (size_t align : {(size_t)16, (size_t)128}) {
        for (size_t elem : {(size_t)2, (size_t)4, (size_t)8}) {
            std::vector<size_t> bytes(k), off(k, (size_t)-1);
            for (size_t i = 0; i < k; i++)
                bytes[i] = n[i] * elem;
            const size_t total = stage_layout(k, bytes.data(), align, off.data());
            // the plain statement: a running end, rounded up by division
            size_t end = 0;
            for (size_t i = 0; i < k; i++) {
                CHECK(off[i] == end && off[i] % align == 0);
                end += (bytes[i] + align - 1) / align * align;
                CHECK(off[i] + bytes[i] <= end && end - (off[i] + bytes[i]) < align);
                if (i + 1 < k)
                    CHECK(off[i + 1] >= off[i] + bytes[i]); // in order, no overlap
            }
            CHECK(total == end);
        }
    }
    // batch_unpacked: uint16 samples at 128 bytes, and the table of the one launch
    std::vector<size_t> bytes(k), off(k);
    for (size_t i = 0; i < k; i++)
        bytes[i] = n[i] * sizeof(uint16_t);
    const size_t total = stage_layout(k, bytes.data(), 128, off.data());
    std::vector<size_t> unpacked_at; // what decoder_stage.hip keeps for adsb_batch_unpacked_copy
    for (size_t i = 0; i < k; i++)
        unpacked_at.push_back(off[i] / sizeof(uint16_t));
    unpacked_at.push_back(total / sizeof(uint16_t));
    for (size_t i = 0; i < k; i++) {
        CHECK(unpacked_at[i + 1] - unpacked_at[i] >= n[i] && unpacked_at[i] % 64 == 0);
        CHECK(unpacked_at[i + 1] - unpacked_at[i] == (n[i] + 63) / 64 * 64); // the capture's slot: its samples rounded up to 128 bytes
    }
    uint64_t groups = ~0ull, want_groups = 0;
    size_t want_rows = 0;
    for (size_t i = 0; i < k; i++)
        want_rows += n[i] != 0;
    if (packed) {
        std::vector<Unpack12Seg> tab(k + 1, Unpack12Seg{~0ull, ~0ull, ~0ull});
        const uint32_t rows = unpack12_table(k, src.data(), n.data(), off.data(), tab.data(), &groups);
        CHECK(rows == want_rows);
        size_t r = 0;
        for (size_t i = 0; i < k; i++) {
            if (n[i] == 0)
                continue;
            CHECK(tab[r].src == (uint64_t)(uintptr_t)src[i] && tab[r].dst16 * 16 == off[i] && tab[r].g_first == want_groups);
            want_groups += n[i] / 8;
            r++;
        }
        CHECK(r == rows && tab[rows].g_first == want_groups && tab[rows].src == 0 && tab[rows].dst16 == 0 && groups == want_groups);
        for (uint32_t q = 0; q + 1 <= rows; q++)
            CHECK(tab[q].g_first < tab[q + 1].g_first); // every row has groups
    } else {
        std::vector<ConvertSeg> tab(k + 1, ConvertSeg{~0ull, ~0ull, ~0ull, ~0ull});
        const uint32_t rows = convert_table(k, src.data(), n.data(), off.data(), tab.data(), &groups);
        CHECK(rows == want_rows);
        size_t r = 0;
        for (size_t i = 0; i < k; i++) {
            if (n[i] == 0)
                continue;
            CHECK(tab[r].src == (uint64_t)(uintptr_t)src[i] && tab[r].dst16 * 16 == off[i] && tab[r].g_first == want_groups && tab[r].n == n[i]);
            want_groups += n[i] / 8 + (n[i] % 8 != 0);
            r++;
        }
        CHECK(r == rows && tab[rows].g_first == want_groups && tab[rows].src == 0 && tab[rows].dst16 == 0 && tab[rows].n == 0 &&
              groups == want_groups);
        for (uint32_t q = 0; q + 1 <= rows; q++)
            CHECK(tab[q].g_first < tab[q + 1].g_first);
    }
    rows_seen += want_rows;
    empties_seen += k - want_rows;
    return true;
}

int main()
{
    std::mt19937_64 rng(20261020);
    for (int packed = 0; packed <= 1; packed++) {
        const size_t unit = packed ? 8 : 1; // packed captures come in whole groups
        std::vector<std::vector<size_t>> lists = {
            {},
            {0},
            {0, 0, 0},
            {0, unit, 0, 0, 2 * unit, 0},                        // empty captures first, last and adjacent
            {unit, 8ull << 29, 0, unit, (8ull << 29) - (packed ? 0 : 15), 0},
            {1 * unit, 2 * unit, 3 * unit, 4 * unit, 5 * unit, 6 * unit, 7 * unit, 8 * unit, 9 * unit},
        };
        for (int t = 0; t < 60; t++) {
            std::vector<size_t> n;
            const int k = 1 + (int)(rng() % 300);
            for (int i = 0; i < k; i++) {
                const unsigned kind = (unsigned)(rng() % 16);
                n.push_back(unit * (kind < 4 ? 0 : kind < 10 ? 1 + rng() % 9 : kind < 15 ? 1 + rng() % 200000 : (1ull << 29) * (packed ? 1 : 8) - rng() % 2));
            }
            lists.push_back(n);
        }
        for (const auto &n : lists) {
            list_no++;
            if (!check_list(n, packed != 0))
                return 1;
        }
    }
    if (rows_seen < 10000 || empties_seen < 3000) {
        printf("only %llu rows and %llu empty captures seen\n", (unsigned long long)rows_seen, (unsigned long long)empties_seen);
        return 1;
    }
    printf("ok: %d lists, %llu rows, %llu empty captures\n", list_no, (unsigned long long)rows_seen, (unsigned long long)empties_seen);
    return 0;
}
