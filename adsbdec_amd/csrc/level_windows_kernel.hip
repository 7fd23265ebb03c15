// level_windows_kernel.hip -- the level reports of K consecutive WINDOWS of one stream by ONE launch (include/adsbdec_amd.h:
// adsb_level_windows; decoder_level_windows.hip).  Window i gets exactly the counts of the power samples [e[i], e[i + 1]) of the
// stream and of the codes of their own pairs, and one envelope serves all windows: every quantity is a count or an unsigned
// maximum, so any order of reduction gives the same bits (adsbdec_amd/levels.py level_windows is the definition).
//
// A sibling of level_batch_kernel.hip, and the same walk: the passes of all windows are numbered in one space (level_windows.hpp), a
// wave takes a contiguous range of them (level_wave_range), the row a pass lies in is found by scalar loads from a table read
// through the constant address space (export_row, the search starting at the previous row), the wave's histogram in LDS belongs to
// ONE window at a time and is flushed to that window's totals when the row changes and at the wave's end, and the four waves of a
// workgroup leave as one sum where they end in the same window.  DESIGN.md section 4 "Batch level report" has what that walk was
// measured against (a grid-stride walk, waves flushing alone); none of it is tried again here.
//
// What differs from the batch unit: the samples, the pairs held and the envelope are the LAUNCH's, not the row's.  Every window
// reads the same buffer, so a pass at a window's start sees the stream's six older pairs, not silence: the front end is
// scan_stages.h real_front as power_export_kernel calls it -- real_front<false>(xin, pbuf0, p_lo = pbuf0, p_hi, w0 - 8, ..) with
// w0 = m_begin + pass * 1792 an ABSOLUTE power sample of the stream, a multiple of 28 -- and a pair outside [pbuf0, p_hi) reads as
// silence pair by pair (adsb_power_window's rule 2).  A pass whose window [w0 - 8, w0 + 1800) lies inside the buffer takes the 17
// typed loads, any other the plain-load road that checks every pair: nothing outside the buffer is ever read.  The envelope float
// of the run at power sample m is env[(m - env0) / 28], env0 the first window's first sample.  A lane's rails are the pairs it
// owns, so a window's rail counters are those of the codes x[2 e[i] : 2 e[i + 1]]; a stream's trailing n % 4 codes belong to no
// window.  The reduction tail (level_tail.h: level_tail, rails_real) is the single unit's and the batch unit's, and the flush
// (level_flush.h: wave_flush, block_finish) the batch unit's: shared, not copied.
#include "scan_stages.h"

#include <algorithm>

#include "level.h"
#include "level_tail.h"
#include "level_flush.h"
#include "level_windows.hpp"

namespace adsb {

namespace {

typedef const __attribute__((address_space(4))) WindowSeg *const_table;

static_assert((uint64_t)kWavePass == kLevelPass, "level_batch.hpp restates the pass of scan_kernel.h's run");
static_assert(ADSB_LEVEL_HIST == 5, "the windows unit is built around a histogram per wave with the run-uniform shortcut");

// q, rem: level_wave_split of the launch's passes over its waves (a kernel has no 64-bit division to do)
__global__ __launch_bounds__(kThreads) void level_windows_kernel(const uint32_t *__restrict__ xin, const int64_t pbuf0, const int64_t p_hi,
                                                                 const int64_t env0, const WindowSeg *__restrict__ tab_in, const uint32_t n_rows,
                                                                 const uint64_t q, const uint64_t rem, unsigned long long *__restrict__ totals,
                                                                 float *__restrict__ env)
{
    __shared__ uint32_t hist[kWaves][kLevelBins];
    __shared__ uint32_t who[kWaves];
    const const_table tab = (const_table)(uintptr_t)tab_in;
    const int lane = threadIdx.x & 63;
    const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t *my_hist = hist[wave_in_block];
    wave_begin(my_hist, lane);
    Counts c;
    uint64_t unit, end;
    level_wave_range(q, rem, (uint64_t)blockIdx.x * kWaves + wave_in_block, &unit, &end);
    uint32_t r = 0;    // the row of the wave's last pass: passes ascend, so the next row is never below it
    bool held = false; // the wave holds counts of row r
#pragma unroll 1
    for (; unit < end; unit++) {
        // the window this pass belongs to (wave-uniform: the scalar unit's)
        const uint32_t rn = export_row(tab, r, n_rows - 1, unit);
        if (rn != r && held)
            wave_flush(my_hist, c, totals + (size_t)tab[r].tot * kLevelWords, lane);
        r = rn, held = true;
        const int64_t m_end = (int64_t)tab[r].m_end;
        const int64_t w0 = (int64_t)tab[r].m_begin + (int64_t)(unit - tab[r].first) * kWavePass; // the wave's first power sample, of the stream
        f32x2 vv[34];
        float a[kRun];
        real_front<false>(xin, pbuf0, pbuf0, p_hi, w0 - 8, lane, vv, a); // (the wave's window starts 8 pairs below)

        // the lane's run is power samples [m0, m0 + 28) of the stream, of which those below the window's end are the window's; the
        // lane owns their pairs, slots 6 .. 33
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
            env[(w0 - env0) / kRun + lane] = __builtin_bit_cast(float, mx);
    }
    block_finish(hist, who, c, held, (uint32_t)tab[r].tot, totals, lane, wave_in_block);
}

} // namespace

hipError_t launch_level_windows(const uint32_t *x, int64_t pbuf0, int64_t p_hi, int64_t env0, const WindowSeg *tab_device, uint32_t n_rows,
                                uint64_t units, unsigned long long *totals, float *env, unsigned max_blocks, hipStream_t stream)
{
    if (units == 0 || n_rows == 0)
        return hipSuccess;
    // as launch_level_batch: 8 workgroups of 256 lanes per CU at most (2048 on the 256 CUs of an MI355X) stream HBM
    const unsigned blocks = (unsigned)std::min<uint64_t>(max_blocks ? max_blocks : 2048, (units + kWaves - 1) / kWaves);
    uint64_t q, rem;
    level_wave_split(units, (uint64_t)blocks * kWaves, &q, &rem);
    hipLaunchKernelGGL(level_windows_kernel, dim3(blocks), dim3(kThreads), 0, stream, x, pbuf0, p_hi, env0, tab_device, n_rows, q, rem, totals, env);
    return hipGetLastError();
}

} // namespace adsb
