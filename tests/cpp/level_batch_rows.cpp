// level_batch_rows.cpp -- csrc/level_batch.hpp on the CPU (tests/test_level_batch_cpu.py builds it with
// -fsanitize=address,undefined and runs it): level_table builds the table the host side uploads, export_row is the look-up the
// kernels make, level_wave_range is how a launch's passes go to its waves.  For seeded lists of capture lengths -- around 0, one
// run, one pass and several passes, with empty captures between them -- every unit must map to the capture that owns it and to the
// right pass inside it; the ranges of 1, 4 and 8192 waves must cover every unit exactly once, in order; and the walk a wave makes
// in level_batch_kernel.hip (search from the previous row, flush when the row changes and at the end), emulated on integer arrays
// with SMALL counters, must leave in every capture's totals exactly what a direct count leaves.  The grid-stride walk of the
// measurement build goes through the same emulation.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../adsbdec_amd/csrc/level_batch.hpp"

using namespace adsb;

static int fail(const char *what, size_t list, uint64_t at)
{
    std::printf("FAILED: %s (list %zu, at %llu)\n", what, list, (unsigned long long)at);
    return 1;
}

constexpr int kBins = 16;          // the emulation's histogram
constexpr uint64_t kRunLen = 28;   // power samples of a run: an envelope float

// the bin of power sample s of capture i: any function of both will do, as long as neighbours differ
static int bin_of(size_t i, uint64_t s) { return (int)((i * 7 + s / 3 + (s >> 9)) % kBins); }

struct Batch {
    std::vector<uint64_t> n, m, p_hi, tail;
    std::vector<const void *> src;
    std::vector<float *> env;
    std::vector<LevelSeg> tab;
    std::vector<uint32_t> row_of;
    uint32_t rows = 0;
    uint64_t units = 0;
};

static Batch make(const std::vector<uint64_t> &n, bool with_env)
{
    Batch b;
    const size_t k = n.size();
    b.n = n;
    b.m.resize(k), b.p_hi.resize(k), b.tail.resize(k), b.src.resize(k), b.env.resize(k), b.tab.resize(k + 1), b.row_of.resize(k);
    for (size_t i = 0; i < k; i++) {
        b.m[i] = 2 * (n[i] / 4);
        b.p_hi[i] = n[i] / 2;
        b.tail[i] = n[i] % 4;
        b.src[i] = reinterpret_cast<const void *>((uintptr_t)(0x1000 + 16 * i)); // (never dereferenced: a capture's name)
        b.env[i] = with_env && i % 3 ? reinterpret_cast<float *>((uintptr_t)(0x80000000u + 4 * i)) : nullptr;
    }
    b.rows = level_table(k, b.m.data(), b.p_hi.data(), b.tail.data(), b.src.data(), with_env ? b.env.data() : nullptr, b.tab.data(), b.row_of.data(),
                         &b.units);
    return b;
}

// the table against a walk over the captures: every unit -> its capture and in-capture pass
static int check_table(size_t list, const Batch &b, uint64_t *units_seen)
{
    const size_t k = b.n.size();
    uint64_t want_units = 0;
    uint32_t want_rows = 0;
    for (size_t i = 0; i < k; i++) {
        want_units += (b.m[i] + kLevelPass - 1) / kLevelPass;
        want_rows += b.m[i] != 0;
    }
    if (b.rows != want_rows || b.units != want_units)
        return fail("rows or units", list, b.rows);
    const LevelSeg &z = b.tab[b.rows];
    if (z.first != b.units || z.src || z.env || z.m_end || z.tail)
        return fail("the closing row", list, b.rows);
    uint64_t unit = 0;
    uint32_t row = 0;
    for (size_t i = 0; i < k; i++) {
        if (b.m[i] == 0) {
            if (b.row_of[i] != UINT32_MAX)
                return fail("an empty capture has a row", list, i);
            continue;
        }
        const LevelSeg &s = b.tab[row];
        if (b.row_of[i] != row || s.tot != row || s.src != (uint64_t)(uintptr_t)b.src[i] || s.env != (uint64_t)(uintptr_t)(b.env[i]) ||
            s.first != unit || s.p_hi != b.p_hi[i] || s.m_end != b.m[i] || s.tail != b.n[i] % 4)
            return fail("a row's fields", list, i);
        const uint64_t np = (b.m[i] + kLevelPass - 1) / kLevelPass;
        for (uint64_t p = 0; p < np; p++, unit++) {
            const uint32_t r = export_row(b.tab.data(), 0, b.rows - 1, unit);
            if (r != row || unit - b.tab[r].first != p)
                return fail("a unit maps to the wrong capture or pass", list, unit);
            if (p * kLevelPass >= b.tab[r].m_end || (p + 1 < np && (p + 1) * kLevelPass > b.tab[r].m_end))
                return fail("a pass outside its capture", list, unit);
        }
        row++;
    }
    *units_seen += unit;
    return unit == b.units ? 0 : fail("the walk's total", list, unit);
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

// What the kernels do, on integers: a wave's small histogram belongs to one row at a time.  stride == 0: the wave's contiguous range;
// else the grid-stride walk of the measurement build.
static int check_flush(size_t list, const Batch &b, uint64_t n_waves, bool stride)
{
    const size_t k = b.n.size();
    if (b.rows == 0)
        return 0;
    std::vector<uint64_t> totals((size_t)b.rows * (kBins + 1), 0), direct((size_t)b.rows * (kBins + 1), 0);
    std::vector<std::vector<uint8_t>> env_hits(k);
    for (size_t i = 0; i < k; i++) {
        env_hits[i].assign((b.m[i] + kRunLen - 1) / kRunLen, 0);
        if (b.row_of[i] == UINT32_MAX)
            continue;
        uint64_t *t = &direct[(size_t)b.row_of[i] * (kBins + 1)];
        for (uint64_t s = 0; s < b.m[i]; s++)
            t[bin_of(i, s)]++;
        t[kBins] = b.n[i] % 4; // the trailing codes, counted once
    }
    std::vector<size_t> capture_of_row(b.rows);
    for (size_t i = 0; i < k; i++)
        if (b.row_of[i] != UINT32_MAX)
            capture_of_row[b.row_of[i]] = i;
    uint64_t q, rem, flushes = 0;
    level_wave_split(b.units, n_waves, &q, &rem);
    for (uint64_t w = 0; w < n_waves; w++) {
        uint64_t unit, end, step = 1;
        if (stride)
            unit = w, end = b.units, step = n_waves;
        else
            level_wave_range(q, rem, w, &unit, &end);
        uint16_t hist[kBins] = {0}; // SMALL counters: a pass adds 1792 at most, and a wave that never flushed would wrap them
        uint64_t tails = 0;
        uint32_t r = 0;
        bool held = false;
        auto flush = [&]() {
            uint64_t *t = &totals[(size_t)b.tab[r].tot * (kBins + 1)];
            for (int j = 0; j < kBins; j++)
                t[j] += hist[j], hist[j] = 0;
            t[kBins] += tails, tails = 0;
            flushes++;
        };
        for (; unit < end; unit += step) {
            const uint32_t rn = export_row(b.tab.data(), r, b.rows - 1, unit);
            if (rn != r && held)
                flush();
            r = rn, held = true;
            const size_t i = capture_of_row[r];
            const uint64_t pass = unit - b.tab[r].first, m_end = b.tab[r].m_end, w0 = pass * kLevelPass;
            for (uint64_t s = w0; s < w0 + kLevelPass && s < m_end; s++) {
                if (hist[bin_of(i, s)] == UINT16_MAX)
                    return fail("a small counter wrapped", list, unit);
                hist[bin_of(i, s)]++;
                if (s % kRunLen == 0)
                    env_hits[i][s / kRunLen]++;
            }
            if (b.tab[r].tail && w0 + kLevelPass >= m_end)
                tails += b.tab[r].tail;
        }
        if (held)
            flush();
    }
    if (totals != direct)
        return fail(stride ? "grid-stride: the totals differ from a direct count" : "ranges: the totals differ from a direct count", list, n_waves);
    for (size_t i = 0; i < k; i++)
        for (uint8_t h : env_hits[i])
            if (h != 1)
                return fail("a run's envelope is not written exactly once", list, i);
    // with ranges a wave flushes once per capture it touches: rows + waves at most
    if (!stride && flushes > (uint64_t)b.rows + n_waves)
        return fail("more flushes than captures and waves", list, flushes);
    return 0;
}

int main()
{
    std::mt19937_64 rng(2053);
    const uint64_t W = 2 * kLevelPass; // 3584 samples: a pass
    uint64_t units = 0;
    size_t lists = 0;
    auto pick = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo + 1); };
    for (; lists < 60; lists++) {
        const size_t k = lists < 4 ? lists : lists % 40 == 0 ? 700 : (size_t)pick(1, 48);
        std::vector<uint64_t> n;
        for (size_t i = 0; i < k; i++) {
            const uint64_t kind = rng() % 8, mult = W * pick(1, 5);
            n.push_back(kind == 0 ? pick(0, 7) : kind == 1 ? pick(52, 60) : kind == 2 ? mult : kind == 3 ? mult + pick(1, 4) : kind == 4 ? mult - pick(1, 4)
                        : kind == 5 ? pick(8, 2 * W) : kind == 6 ? W + pick(0, 3) : pick(1, 8 * W));
            if (rng() % 2)
                n.push_back(rng() % 4); // an empty capture between two
        }
        const Batch b = make(n, lists % 2 == 0);
        if (check_table(lists, b, &units))
            return 1;
        for (uint64_t waves : {1ull, 4ull, 8192ull}) {
            if (check_ranges(lists, b.units, waves) || check_flush(lists, b, waves, false))
                return 1;
            if (waves != 8192 && check_flush(lists, b, waves, true))
                return 1;
        }
    }
    // every capture empty; every capture exactly one pass; units in numbers the waves do not divide
    const Batch none = make(std::vector<uint64_t>(33, 3), true), ones = make(std::vector<uint64_t>(300, W), false);
    if (check_table(lists++, none, &units) || check_flush(lists, none, 4, false) || check_table(lists++, ones, &units) || check_flush(lists, ones, 4, false))
        return 1;
    for (uint64_t u : {0ull, 1ull, 3ull, 8191ull, 8192ull, 8193ull, (1ull << 53) + 12345})
        for (uint64_t waves : {1ull, 4ull, 8192ull})
            if (check_ranges(lists, u, waves))
                return 1;
    std::printf("ok: %zu lists, %llu units\n", lists, (unsigned long long)units);
    return 0;
}
