// level_windows.hpp -- the table of level_windows_kernel.hip (include/adsbdec_amd.h: adsb_level_windows, adsb_level_windows_host).
// Host + device code: the row search (power_export_batch.hpp export_row) and the split of the passes over the waves
// (level_batch.hpp level_wave_range) are the kernel's and the CPU test's (tests/cpp/level_windows_rows.cpp); building the table is
// host-only.
//
// ONE stream, K consecutive windows of its power samples: edges e[0] <= e[1] <= ... <= e[K], window i = [e[i], e[i + 1]), every edge
// but the last a multiple of 28 -- so a run of 28 (a lane's work, an envelope float) never spans two windows.  The passes of all
// windows are numbered in ONE space, window after window, as the batch level report numbers the passes of its captures: window i
// owns ceil((e[i + 1] - e[i]) / 1792) consecutive pass numbers, its pass p starts at power sample e[i] + 1792 p of the STREAM, and a
// pass never spans two windows.  A row per window THAT HAS POWER SAMPLES, in window order (an empty window has no row and costs
// nothing); the row behind the last one holds the total.  What the batch's row carries per capture -- samples, pairs held, envelope
// -- is the launch's here: every window reads the same buffer, and one envelope serves all of them.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "level_batch.hpp" // export_row, export_units, kLevelPass, kLevelBatchCaptures, level_wave_range, level_wave_split

namespace adsb {

struct WindowSeg {
    uint64_t first;   // the window's first pass's number; in the closing row: the number of all passes
    uint64_t m_begin; // its first power sample, of the stream: a multiple of 28
    uint64_t m_end;   // the power sample behind its last, anywhere above m_begin
    uint64_t tot;     // which of the launch's totals are the window's: words [tot * kLevelWords, + kLevelWords)
};

// ---- host-only: building the table ----
// The table of the n_windows windows between edges[0 .. n_windows] into tab[0 .. rows], rows <= n_windows.  row_of[i] = window i's
// row, = its totals, or UINT32_MAX where it is empty.  *units = the number of all passes.  Returns the rows, the closing one not
// counted.
inline uint32_t level_windows_table(size_t n_windows, const uint64_t *edges, WindowSeg *tab, uint32_t *row_of, uint64_t *units)
{
    uint32_t row = 0;
    uint64_t at = 0;
    for (size_t i = 0; i < n_windows; i++) {
        row_of[i] = UINT32_MAX;
        if (edges[i + 1] <= edges[i])
            continue;
        row_of[i] = row;
        tab[row] = WindowSeg{at, edges[i], edges[i + 1], row};
        row++;
        at += export_units(edges[i + 1] - edges[i], kLevelPass);
    }
    tab[row] = WindowSeg{at, 0, 0, 0};
    *units = at;
    return row;
}

#ifdef __HIPCC__
// level_windows_kernel.hip: the n_rows windows of the table at tab_device (device memory), `units` passes in all, over the uint16
// samples at x -- x[0] is pair pbuf0 of the stream, the pairs [pbuf0, p_hi) are held, every other pair reads as silence -- reduced
// into totals (n_rows x kLevelWords uint64 in device memory, zeroed by the caller on the same stream; the counts are ADDED), the
// maximum of the run at power sample env0 + 28 r written to env[r] (env == NULL: none).  Enqueued on `stream` behind the table's
// upload.  max_blocks: 0, or the most workgroups the launch may have (adsb_debug_set_level_batch_blocks).  Nothing is launched for
// a table without units.
hipError_t launch_level_windows(const uint32_t *x, int64_t pbuf0, int64_t p_hi, int64_t env0, const WindowSeg *tab_device, uint32_t n_rows,
                                uint64_t units, unsigned long long *totals, float *env, unsigned max_blocks, hipStream_t stream);
#endif

} // namespace adsb
