// level_batch_kernel.hip -- the level reports of a BATCH of captures by ONE launch (include/adsbdec_amd.h: the adsb_level_batch_*
// calls; decoder_level_batch.hip).  Capture i gets exactly the counts, and where asked the envelope, that level_kernel.hip gives
// it alone: every quantity is a count or an unsigned maximum, so any order of reduction gives the same bits.
//
// level_batch_kernel is level_kernel's body with the capture looked up per pass, the way power_export_batch_kernel does it: the
// passes of all captures are numbered in one space (level_batch.hpp), a wave's pass number is wave-uniform, the row it lies in is
// found by scalar loads from a table read through the constant address space, and with the row in hand the body is
// level_kernel's with the row's p_hi, m_end, samples and envelope -- every capture a fresh stream whose six pairs in front of pair
// 0 read as silence whatever lies in front of it in memory.  The front end is scan_stages.h real_front, called as the batch
// export calls it (s_nop 4 in front of its typed loads: the descriptor comes from a table row read per pass); a capture's first
// pass takes its plain-load road (the window starts 8 pairs below pair 0).  level_units_batch_kernel<kKind> is level_units_kernel's
// body for complex int16, complex int8 and float32 power input over the same table; its 16 / 8-byte loads are taken where THAT
// capture's pointer is aligned for them.  The tail (level_tail.h) is the single unit's, shared, not copied.
//
// Accumulation.  A histogram per wave in LDS with the run-uniform shortcut, as the single unit ships it (8 KiB a wave, 32 KiB a
// workgroup, five workgroups per CU) -- but the histogram belongs to ONE capture at a time: when the wave's row changes, and at
// the wave's end, the wave adds its non-zero bins and its counters to the totals of the capture it held (masked 64-bit vector
// atomics, 32 wave-instructions of 512 contiguous bytes) and zeroes what it added.  Nothing crosses waves while they walk: no
// workgroup barrier per pass, no counters in LDS.  At the END the four waves of a workgroup meet once (block_finish): where all
// four hold the same capture -- every workgroup inside a long capture -- their histograms leave as ONE sum, as the single kernel's
// do; 8192 waves adding the same few hundred words of one capture one after the other is what a batch of one large capture
// otherwise ends on (ADSB_LEVEL_BATCH_MERGE=0 in a measurement build: every wave flushes alone).  The flush is level_flush.h's,
// shared with level_windows_kernel.hip.  32-bit LDS counts cannot
// overflow (a capture has fewer than 2^32 power samples).
// ADSB_LEVEL_BATCH_WALK picks how the passes go to the waves in a measurement build (the shipped one defines nothing; DESIGN.md
// section 4 "Batch level report" has the numbers):
//   0  a contiguous range of passes per wave (level_wave_range): a row change is as rare as a capture's end, a capture of k passes
//      is flushed by ceil(k / range) + 1 waves at most, and the search for the next row starts at the previous one.  Shipped.
//   1  grid-stride, as the single kernel walks: neighbouring passes of a wave are gridDim x 4 apart, so in a batch of short
//      captures the row changes -- and the wave flushes -- on every pass.
//
// A real capture's trailing n % 4 codes make no power sample, but the rail counters are the capture's: the wave that takes the
// capture's last pass loads them (row.tail of them, at sample 2 m_end) and counts them, so a batch issues no copy per capture.
#include "scan_stages.h"

#include <algorithm>

#include "level.h"
#include "level_tail.h"
#include "level_flush.h" // wave_begin, wave_flush, block_finish: shared with level_windows_kernel.hip
#include "level_batch.hpp"

#ifndef ADSB_LEVEL_BATCH_WALK
#define ADSB_LEVEL_BATCH_WALK 0
#endif

namespace adsb {

namespace {

typedef const __attribute__((address_space(4))) LevelSeg *const_table;
typedef const __attribute__((address_space(1))) uint32_t *global_words;
typedef const __attribute__((address_space(1))) uint16_t *global_halves;
typedef const __attribute__((address_space(1))) u32x4 *global_u32x4;
typedef const __attribute__((address_space(1))) u32x2 *global_u32x2;
typedef __attribute__((address_space(1))) float *global_floats;

static_assert((uint64_t)kWavePass == kLevelPass, "level_batch.hpp restates the pass of scan_kernel.h's run");
static_assert(ADSB_LEVEL_HIST == 5, "the batch unit is built around a histogram per wave with the run-uniform shortcut");

// The passes of wave w of n_waves: from *u on, below *end, `step` apart (wave-uniform).
struct Walk {
    uint64_t units, q, rem; // all passes; level_wave_split of them over the launch's waves
};
__device__ __forceinline__ void wave_walk(const Walk &k, const uint64_t n_waves, const uint64_t w, uint64_t *u, uint64_t *end, uint64_t *step)
{
#if ADSB_LEVEL_BATCH_WALK == 0
    level_wave_range(k.q, k.rem, w, u, end);
    *step = 1;
#else
    *u = w, *end = k.units, *step = n_waves;
#endif
}

__global__ __launch_bounds__(kThreads) void level_batch_kernel(const LevelSeg *__restrict__ tab_in, const uint32_t n_rows, const Walk walk,
                                                               unsigned long long *__restrict__ totals)
{
    __shared__ uint32_t hist[kWaves][kLevelBins];
    __shared__ uint32_t who[kWaves];
    const const_table tab = (const_table)(uintptr_t)tab_in;
    const int lane = threadIdx.x & 63;
    const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t *my_hist = hist[wave_in_block];
    wave_begin(my_hist, lane);
    Counts c;
    uint64_t unit, end, step;
    wave_walk(walk, (uint64_t)gridDim.x * kWaves, (uint64_t)blockIdx.x * kWaves + wave_in_block, &unit, &end, &step);
    uint32_t r = 0;    // the row of the wave's last pass: units ascend, so the next row is never below it
    bool held = false; // the wave holds counts of row r
#pragma unroll 1
    for (; unit < end; unit += step) {
        // the capture this pass belongs to, and the pass's number inside it (wave-uniform: the scalar unit's)
        const uint32_t rn = export_row(tab, r, n_rows - 1, unit);
        if (rn != r && held)
            wave_flush(my_hist, c, totals + (size_t)tab[r].tot * kLevelWords, lane);
        r = rn, held = true;
        const int64_t pass = (int64_t)(unit - tab[r].first);
        const int64_t p_hi = (int64_t)tab[r].p_hi, m_end = (int64_t)tab[r].m_end;
        const global_words xin = (global_words)tab[r].src;
        const global_floats env = (global_floats)tab[r].env;
        const int64_t w0 = pass * kWavePass; // the wave's first power sample = lane 0's first pair: a multiple of 28
        f32x2 vv[34];
        float a[kRun];
        real_front<true>(xin, 0, 0, p_hi, w0 - 8, lane, vv, a); // (the wave's window starts 8 pairs below: never interior in a capture's first pass)

        // the lane's run is power samples [m0, m0 + 28) of the capture, of which those below m_end exist; the lane owns their pairs
        const int64_t m0 = w0 + (int64_t)kRun * lane;
        const int left = (int)std::min<int64_t>(kRun, std::max<int64_t>(0, m_end - m0));
        const bool full = w0 + kWavePass <= m_end; // (wave-uniform)
        uint32_t b[kRun];
#pragma unroll
        for (int k = 0; k < kRun; k++)
            b[k] = __builtin_bit_cast(uint32_t, a[k]);
        const uint32_t mx = full ? level_tail<true, false>(b, kRun, my_hist, c, lane) : level_tail<false, false>(b, left, my_hist, c, lane);
        if (full)
            rails_real<true>(vv, kRun, c);
        else
            rails_real<false>(vv, left, c);
        if (env && left > 0)
            env[pass * 64 + lane] = __builtin_bit_cast(float, mx);
        // the capture's last pass: the codes behind its last whole group of four, samples 2 m_end .. of the n it holds
        const int tail = (int)tab[r].tail;
        if (tail && w0 + kWavePass >= m_end) { // (wave-uniform)
            const bool mine = lane < tail;
            const uint32_t code = mine ? (uint32_t)((global_halves)xin)[2 * m_end + lane] : 1u;
            c.rail_lo += lanes(mine && code == 0u);
            c.rail_hi += lanes(mine && code == 4095u);
            c.over += lanes(mine && code > 4095u);
        }
    }
    block_finish(hist, who, c, held, (uint32_t)tab[r].tot, totals, lane, wave_in_block);
}

template <int kKind>
__global__ __launch_bounds__(kThreads) void level_units_batch_kernel(const LevelSeg *__restrict__ tab_in, const uint32_t n_rows, const Walk walk,
                                                                     unsigned long long *__restrict__ totals)
{
    __shared__ uint32_t hist[kWaves][kLevelBins];
    __shared__ uint32_t who[kWaves];
    const const_table tab = (const_table)(uintptr_t)tab_in;
    const int lane = threadIdx.x & 63;
    const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t *my_hist = hist[wave_in_block];
    wave_begin(my_hist, lane);
    Counts c;
    uint64_t unit, end, step;
    wave_walk(walk, (uint64_t)gridDim.x * kWaves, (uint64_t)blockIdx.x * kWaves + wave_in_block, &unit, &end, &step);
    uint32_t r = 0;
    bool held = false;
    constexpr size_t kUnit = kKind == kLevelIq8 ? 2 : 4;
#pragma unroll 1
    for (; unit < end; unit += step) {
        const uint32_t rn = export_row(tab, r, n_rows - 1, unit);
        if (rn != r && held)
            wave_flush(my_hist, c, totals + (size_t)tab[r].tot * kLevelWords, lane);
        r = rn, held = true;
        const size_t pass = (size_t)(unit - tab[r].first), n = (size_t)tab[r].m_end;
        const uint64_t src = tab[r].src;
        const global_floats env = (global_floats)tab[r].env;
        const bool aligned = src % (4 * kUnit) == 0; // (wave-uniform; a run is 28 units: every lane's is then aligned as the capture is)
        const size_t w0 = pass * kWavePass, m0 = w0 + (size_t)kRun * lane;
        const bool full = w0 + kWavePass <= n; // (wave-uniform)
        const int left = m0 >= n ? 0 : (int)std::min<size_t>(kRun, n - m0);
        uint32_t u[kRun];
        if (full && aligned) {
            if constexpr (kKind == kLevelIq8) {
                const global_u32x2 p = (global_u32x2)((global_halves)src + m0);
#pragma unroll
                for (int k = 0; k < kRun / 4; k++) {
                    const u32x2 q = p[k];
                    u[4 * k] = q.x & 0xFFFFu, u[4 * k + 1] = q.x >> 16, u[4 * k + 2] = q.y & 0xFFFFu, u[4 * k + 3] = q.y >> 16;
                }
            } else {
                const global_u32x4 p = (global_u32x4)((global_words)src + m0);
#pragma unroll
                for (int k = 0; k < kRun / 4; k++) {
                    const u32x4 q = p[k];
                    u[4 * k] = q.x, u[4 * k + 1] = q.y, u[4 * k + 2] = q.z, u[4 * k + 3] = q.w;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < kRun; k++) {
                u[k] = 0;
                if (k < left)
                    u[k] = kKind == kLevelIq8 ? (uint32_t)((global_halves)src)[m0 + k] : ((global_words)src)[m0 + k];
            }
        }
        uint32_t b[kRun];
#pragma unroll
        for (int k = 0; k < kRun; k++)
            b[k] = unit_bits<kKind>(u[k]);
        constexpr bool kSigned = kKind == kLevelPower;
        const uint32_t mx = full ? level_tail<true, kSigned>(b, kRun, my_hist, c, lane) : level_tail<false, kSigned>(b, left, my_hist, c, lane);
        if constexpr (kKind != kLevelPower) {
            if (full)
                rails_iq<kKind, true>(u, kRun, c);
            else
                rails_iq<kKind, false>(u, left, c);
        }
        if (env && left > 0)
            env[pass * 64 + lane] = __builtin_bit_cast(float, mx);
    }
    block_finish(hist, who, c, held, (uint32_t)tab[r].tot, totals, lane, wave_in_block);
}

} // namespace

hipError_t launch_level_batch(int kind, const LevelSeg *tab_device, uint32_t n_rows, uint64_t units, unsigned long long *totals,
                              unsigned max_blocks, hipStream_t stream)
{
    if (units == 0 || n_rows == 0)
        return hipSuccess;
    // as launch_level: 8 workgroups of 256 lanes per CU at most (2048 on the 256 CUs of an MI355X) stream HBM
    const unsigned blocks = (unsigned)std::min<uint64_t>(max_blocks ? max_blocks : 2048, (units + kWaves - 1) / kWaves);
    const dim3 g(blocks), b(kThreads);
    Walk walk{units, 0, 0};
    level_wave_split(units, (uint64_t)blocks * kWaves, &walk.q, &walk.rem);
    if (kind == kLevelIq16)
        hipLaunchKernelGGL(level_units_batch_kernel<kLevelIq16>, g, b, 0, stream, tab_device, n_rows, walk, totals);
    else if (kind == kLevelIq8)
        hipLaunchKernelGGL(level_units_batch_kernel<kLevelIq8>, g, b, 0, stream, tab_device, n_rows, walk, totals);
    else if (kind == kLevelPower)
        hipLaunchKernelGGL(level_units_batch_kernel<kLevelPower>, g, b, 0, stream, tab_device, n_rows, walk, totals);
    else
        hipLaunchKernelGGL(level_batch_kernel, g, b, 0, stream, tab_device, n_rows, walk, totals);
    return hipGetLastError();
}

} // namespace adsb
