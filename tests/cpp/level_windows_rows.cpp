// level_windows_rows.cpp -- csrc/level_windows.hpp on the CPU (tests/test_level_windows_cpu.py builds it with
// -fsanitize=address,undefined and runs it): level_windows_table builds the table the host side uploads, export_row is the look-up
// the kernel makes, level_wave_range is how a launch's passes go to its waves.  For seeded edge lists -- windows of 28, of one pass,
// of several passes, ragged last windows and empty windows between them -- every pass must belong to exactly one window and start
// at the right power sample of the stream, every power sample of [e[0], e[K]) must be covered exactly once, the row of a pass must be
// found from ANY starting row that is not behind it, the ranges of 1, 4, 7 and 8192 waves must cover every pass exactly once, and
// the walk a wave makes in level_windows_kernel.hip (search from the previous row, flush when the row changes and at the end),
// emulated on integer arrays with SMALL counters, must leave in every window's totals exactly what a direct count leaves and write
// every float of the ONE shared envelope exactly once.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../adsbdec_amd/csrc/level_windows.hpp"

using namespace adsb;

static int fail(const char *what, size_t list, uint64_t at)
{
    std::printf("FAILED: %s (list %zu, at %llu)\n", what, list, (unsigned long long)at);
    return 1;
}

constexpr int kBins = 16;        // the emulation's histogram
constexpr uint64_t kRunLen = 28; // power samples of a run: an envelope float

// the bin of power sample s of the stream: any function will do, as long as neighbours differ
static int bin_of(uint64_t s) { return (int)((s / 3 + (s >> 9) + (s >> 13)) % kBins); }

struct Windows {
    std::vector<uint64_t> e;
    std::vector<WindowSeg> tab;
    std::vector<uint32_t> row_of;
    uint32_t rows = 0;
    uint64_t units = 0;
};

static Windows make(const std::vector<uint64_t> &e)
{
    Windows w;
    w.e = e;
    const size_t k = e.size() - 1;
    w.tab.resize(k + 1), w.row_of.resize(k);
    w.rows = level_windows_table(k, e.data(), w.tab.data(), w.row_of.data(), &w.units);
    return w;
}

// the table against a walk over the windows: every pass -> its window and its first power sample; every power sample once
static int check_table(size_t list, const Windows &w, uint64_t *units_seen)
{
    const size_t k = w.e.size() - 1;
    uint64_t want_units = 0;
    uint32_t want_rows = 0;
    for (size_t i = 0; i < k; i++) {
        want_units += (w.e[i + 1] - w.e[i] + kLevelPass - 1) / kLevelPass;
        want_rows += w.e[i + 1] > w.e[i];
    }
    if (w.rows != want_rows || w.units != want_units)
        return fail("rows or units", list, w.rows);
    const WindowSeg &z = w.tab[w.rows];
    if (z.first != w.units || z.m_begin || z.m_end || z.tot)
        return fail("the closing row", list, w.rows);
    uint64_t unit = 0, covered = w.e[0];
    uint32_t row = 0;
    for (size_t i = 0; i < k; i++) {
        if (w.e[i + 1] == w.e[i]) {
            if (w.row_of[i] != UINT32_MAX)
                return fail("an empty window has a row", list, i);
            continue;
        }
        const WindowSeg &s = w.tab[row];
        if (w.row_of[i] != row || s.tot != row || s.first != unit || s.m_begin != w.e[i] || s.m_end != w.e[i + 1] || s.m_begin % kRunLen)
            return fail("a row's fields", list, i);
        const uint64_t np = (w.e[i + 1] - w.e[i] + kLevelPass - 1) / kLevelPass;
        for (uint64_t p = 0; p < np; p++, unit++) {
            for (uint32_t from : {0u, row / 2, row ? row - 1 : 0u, row}) { // any starting row not behind it
                const uint32_t r = export_row(w.tab.data(), from, w.rows - 1, unit);
                if (r != row || unit - w.tab[r].first != p)
                    return fail("a pass maps to the wrong window or number", list, unit);
            }
            const uint64_t w0 = s.m_begin + p * kLevelPass, w1 = w0 + kLevelPass < s.m_end ? w0 + kLevelPass : s.m_end;
            if (w0 != covered || w0 >= s.m_end || w0 % kRunLen)
                return fail("a pass does not start where the one before it ended", list, unit);
            covered = w1;
        }
        row++;
    }
    *units_seen += unit;
    return unit == w.units && covered == w.e[k] ? 0 : fail("the walk's total", list, unit);
}

// the ranges of n_waves waves: in order, gapless, every unit once, sizes one apart at most
static int check_ranges(size_t list, uint64_t units, uint64_t n_waves)
{
    uint64_t q, rem, at = 0, lo = UINT64_MAX, hi = 0;
    level_wave_split(units, n_waves, &q, &rem);
    for (uint64_t w = 0; w < n_waves; w++) {
        uint64_t u0, u1;
        level_wave_range(q, rem, w, &u0, &u1);
        if (u0 != at || u1 < u0)
            return fail("a wave's range does not follow its neighbour's", list, w);
        lo = u1 - u0 < lo ? u1 - u0 : lo, hi = u1 - u0 > hi ? u1 - u0 : hi;
        at = u1;
    }
    if (at != units || hi - lo > 1)
        return fail("the ranges do not cover the units evenly", list, n_waves);
    return 0;
}

// What the kernel does, on integers: a wave's small histogram belongs to one row at a time.
static int check_flush(size_t list, const Windows &w, uint64_t n_waves)
{
    if (w.rows == 0)
        return 0;
    const size_t k = w.e.size() - 1;
    const uint64_t e0 = w.e[0], eK = w.e[k];
    std::vector<uint64_t> totals((size_t)w.rows * kBins, 0), direct((size_t)w.rows * kBins, 0);
    std::vector<uint8_t> env_hits((eK - e0 + kRunLen - 1) / kRunLen, 0);
    for (size_t i = 0; i < k; i++)
        for (uint64_t s = w.e[i]; s < w.e[i + 1]; s++)
            direct[(size_t)w.row_of[i] * kBins + bin_of(s)]++;
    uint64_t q, rem, flushes = 0;
    level_wave_split(w.units, n_waves, &q, &rem);
    for (uint64_t wave = 0; wave < n_waves; wave++) {
        uint64_t unit, end;
        level_wave_range(q, rem, wave, &unit, &end);
        uint16_t hist[kBins] = {0}; // SMALL counters: a pass adds 1792 at most, and a wave that never flushed would wrap them
        uint32_t r = 0;
        bool held = false;
        auto flush = [&]() {
            uint64_t *t = &totals[(size_t)w.tab[r].tot * kBins];
            for (int j = 0; j < kBins; j++)
                t[j] += hist[j], hist[j] = 0;
            flushes++;
        };
        for (; unit < end; unit++) {
            const uint32_t rn = export_row(w.tab.data(), r, w.rows - 1, unit);
            if (rn != r && held)
                flush();
            r = rn, held = true;
            const uint64_t m_end = w.tab[r].m_end, w0 = w.tab[r].m_begin + (unit - w.tab[r].first) * kLevelPass;
            for (int lane = 0; lane < 64; lane++) {
                const uint64_t m0 = w0 + kRunLen * lane;
                if (m0 >= m_end)
                    break;
                const size_t at = (size_t)((w0 - e0) / kRunLen) + lane; // the kernel's index into the shared envelope
                if (at >= env_hits.size())
                    return fail("an envelope float outside the array", list, unit);
                env_hits[at]++;
                for (uint64_t s = m0; s < m0 + kRunLen && s < m_end; s++) {
                    if (hist[bin_of(s)] == UINT16_MAX)
                        return fail("a small counter wrapped", list, unit);
                    hist[bin_of(s)]++;
                }
            }
        }
        if (held)
            flush();
    }
    if (totals != direct)
        return fail("the totals differ from a direct count", list, n_waves);
    for (size_t r = 0; r < env_hits.size(); r++)
        if (env_hits[r] != 1)
            return fail("a run's envelope is not written exactly once", list, r);
    // a wave flushes once per window it touches: rows + waves at most
    if (flushes > (uint64_t)w.rows + n_waves)
        return fail("more flushes than windows and waves", list, flushes);
    return 0;
}

int main()
{
    std::mt19937_64 rng(2827);
    uint64_t units = 0;
    size_t lists = 0;
    auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
    for (; lists < 60; lists++) {
        const size_t k = lists < 4 ? lists + 1 : lists % 30 == 0 ? 1100 : (size_t)pick(1, 64);
        std::vector<uint64_t> e{kRunLen * pick(0, lists % 3 ? 5000 : 0)};
        for (size_t i = 0; i < k; i++) {
            const uint64_t kind = rng() % 8;
            // in runs of 28: nothing, one run, a few runs, one pass, a pass and a run, a run short of two passes, several passes, anything
            const uint64_t runs = kind == 0 ? 0 : kind == 1 ? 1 : kind == 2 ? pick(2, 5) : kind == 3 ? 64 : kind == 4 ? 65 : kind == 5 ? 127 : kind == 6 ? 64 * pick(2, 4) : pick(1, 400);
            e.push_back(e.back() + kRunLen * runs);
        }
        if (lists % 2) // a last edge anywhere: the last window ends inside a run, or is empty
            e.back() = e[e.size() - 2] + pick(0, 3 * kLevelPass);
        const Windows w = make(e);
        if (check_table(lists, w, &units))
            return 1;
        for (uint64_t waves : {1ull, 4ull, 7ull, 8192ull})
            if (check_ranges(lists, w.units, waves) || check_flush(lists, w, waves))
                return 1;
    }
    // every window empty; every window one run; every window exactly one pass
    std::vector<uint64_t> none(34, 28 * 9), runs, passes;
    for (uint64_t i = 0; i <= 1025; i++)
        runs.push_back(28 * (3 + i)), passes.push_back(kLevelPass * i);
    for (const std::vector<uint64_t> &e : {none, runs, passes}) {
        const Windows w = make(e);
        if (check_table(lists, w, &units) || check_flush(lists, w, 4) || check_flush(lists, w, 8))
            return 1;
        lists++;
    }
    std::printf("ok: %zu lists, %llu units\n", lists, (unsigned long long)units);
    return 0;
}
