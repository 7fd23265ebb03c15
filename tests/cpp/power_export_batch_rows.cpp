// power_export_batch_rows.cpp -- csrc/power_export_batch.hpp on the CPU (tests/test_power_export_batch_cpu.py builds it with
// -fsanitize=address,undefined and runs it): export_table builds the table the host side uploads, export_row is the look-up the
// kernels make.  For many randomised lists of capture lengths every pass number must map to the capture that owns it and to the
// right pass inside it; the closing row holds the total; a capture without power samples has no row.  The IQ table (groups of
// four complex samples) is looked up chunk-wise, as iq_power_export_batch_kernel does it.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../adsbdec_amd/csrc/power_export_batch.hpp"

using namespace adsb;

static int fail(const char *what, size_t list, uint64_t at)
{
    std::printf("FAILED: %s (list %zu, at %llu)\n", what, list, (unsigned long long)at);
    return 1;
}

// one list of real captures: every pass against a walk over the captures
static int check_real(size_t list, const std::vector<uint64_t> &n, uint64_t *passes_seen)
{
    const size_t k = n.size();
    std::vector<uint64_t> m(k), p_hi(k);
    std::vector<const void *> src(k);
    std::vector<float *> out(k);
    for (size_t i = 0; i < k; i++) {
        m[i] = 2 * (n[i] / 4);
        p_hi[i] = n[i] / 2;
        src[i] = reinterpret_cast<const void *>((uintptr_t)(0x1000 + 16 * i)); // (never dereferenced: a capture's name)
        out[i] = reinterpret_cast<float *>((uintptr_t)(0x80000000u + 16 * i));
    }
    std::vector<ExportSeg> tab(k + 1);
    uint64_t units = 0;
    const uint32_t rows = export_table(k, m.data(), p_hi.data(), src.data(), out.data(), kExportPass, tab.data(), &units);
    uint64_t want_units = 0;
    uint32_t want_rows = 0;
    for (size_t i = 0; i < k; i++) {
        want_units += (m[i] + kExportPass - 1) / kExportPass;
        want_rows += m[i] != 0;
    }
    if (rows != want_rows || units != want_units)
        return fail("rows or units", list, rows);
    if (tab[rows].first != units || tab[rows].src || tab[rows].out || tab[rows].m_end)
        return fail("the closing row", list, rows);
    if (rows == 0)
        return units == 0 ? 0 : fail("units without rows", list, units);
    uint64_t unit = 0;
    uint32_t row = 0;
    for (size_t i = 0; i < k; i++) {
        if (m[i] == 0)
            continue; // no row: the next capture's row follows the previous one's
        const ExportSeg &s = tab[row];
        if (s.src != (uint64_t)(uintptr_t)src[i] || s.out != (uint64_t)(uintptr_t)out[i] || s.first != unit || s.p_hi != p_hi[i] || s.m_end != m[i])
            return fail("a row's fields", list, i);
        const uint64_t np = (m[i] + kExportPass - 1) / kExportPass;
        for (uint64_t p = 0; p < np; p++, unit++) {
            const uint32_t r = export_row(tab.data(), 0, rows - 1, unit);
            if (r != row || unit - tab[r].first != p)
                return fail("a pass maps to the wrong capture or pass", list, unit);
            // the pass lies inside its capture: it starts below m_end, and only the last one may end behind it
            if (p * kExportPass >= tab[r].m_end || (p + 1 < np && (p + 1) * kExportPass > tab[r].m_end))
                return fail("a pass outside its capture", list, unit);
        }
        row++;
    }
    *passes_seen += unit;
    return unit == units ? 0 : fail("the walk's total", list, unit);
}

// one list of IQ captures: every group, looked up chunk-wise
static int check_iq(size_t list, const std::vector<uint64_t> &n)
{
    const size_t k = n.size();
    std::vector<const void *> src(k);
    std::vector<float *> out(k);
    for (size_t i = 0; i < k; i++) {
        src[i] = reinterpret_cast<const void *>((uintptr_t)(0x1000 + 4 * i));
        out[i] = reinterpret_cast<float *>((uintptr_t)(0x80000000u + 16 * i));
    }
    std::vector<ExportSeg> tab(k + 1);
    uint64_t groups = 0;
    const uint32_t rows = export_table(k, n.data(), nullptr, src.data(), out.data(), kExportIqGroup, tab.data(), &groups);
    if (tab[rows].first != groups)
        return fail("the closing row (IQ)", list, rows);
    if (rows == 0)
        return 0;
    std::vector<uint32_t> owner; // group -> capture, by a walk
    for (size_t i = 0; i < k; i++)
        for (uint64_t g = 0; g < (n[i] + 3) / 4; g++)
            owner.push_back((uint32_t)i);
    if (owner.size() != groups)
        return fail("groups", list, groups);
    for (uint64_t g0 = 0; g0 < groups; g0 += kExportIqChunk) {
        const uint64_t g1 = g0 + (kExportIqChunk - 1) < groups ? g0 + (kExportIqChunk - 1) : groups - 1;
        const uint32_t r0 = export_row(tab.data(), 0, rows - 1, g0), r1 = export_row(tab.data(), r0, rows - 1, g1);
        for (uint64_t g = g0; g <= g1; g++) {
            const uint32_t r = export_row(tab.data(), r0, r1, g);
            const uint64_t at = 4 * (g - tab[r].first);
            if (tab[r].src != (uint64_t)(uintptr_t)src[owner[g]] || at >= tab[r].m_end || tab[r].m_end != n[owner[g]])
                return fail("a group maps to the wrong capture", list, g);
        }
    }
    return 0;
}

int main()
{
    std::mt19937_64 rng(1792);
    const uint64_t W = 2 * kExportPass; // 3584 samples: a pass
    uint64_t passes = 0;
    size_t lists = 0;
    auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
    for (; lists < 300; lists++) {
        const size_t k = lists < 4 ? lists : lists % 25 == 0 ? 2048 : (size_t)pick(1, 96);
        std::vector<uint64_t> n(k);
        for (auto &v : n) {
            const uint64_t kind = rng() % 8, mult = W * pick(1, 6);
            v = kind == 0 ? 0 : kind == 1 ? pick(1, 7) : kind == 2 ? mult : kind == 3 ? mult + pick(1, 4) : kind == 4 ? mult - pick(1, 4)
                : kind == 5 ? pick(8, 2 * W) : kind == 6 ? pick(0, 3) : pick(1, 40 * W);
        }
        if (lists % 100 == 7 && k)
            n[rng() % k] = (1ull << 32) - 4; // the longest capture a batch takes, among short ones
        if (check_real(lists, n, &passes))
            return 1;
        for (auto &v : n)
            v = v > (1u << 20) ? v % 4099 : v; // (IQ: the same lists, the long captures cut)
        if (check_iq(lists, n))
            return 1;
    }
    // every capture empty, and every capture exactly one pass
    std::vector<uint64_t> none(33, 3), ones(300, W);
    if (check_real(lists++, none, &passes) || check_real(lists++, ones, &passes))
        return 1;
    std::printf("ok: %zu lists, %llu passes\n", lists, (unsigned long long)passes);
    return 0;
}
