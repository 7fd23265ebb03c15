// level_batch.hpp -- the table of level_batch_kernel.hip (include/adsbdec_amd.h: the adsb_level_batch_* calls) and the split of its
// units over the waves of a launch.  Host + device code: the row search (power_export_batch.hpp export_row) and the split are the
// kernels' and the CPU test's (tests/cpp/level_batch_rows.cpp); building the table is host-only.
//
// The units of all captures are numbered in ONE space, capture after capture, as the batch export numbers its passes: a unit is a
// PASS -- one wave, 64 runs, 1792 power samples of ONE capture (real captures) or 1792 units that ARE power samples (complex int16,
// complex int8, float32 power).  A capture of m power samples owns ceil(m / 1792) consecutive unit numbers and a pass never spans
// two captures.  A row per capture THAT HAS UNITS, in capture order (a capture without power samples has no row and costs
// nothing); the row behind the last one holds the total.
//
// A wave takes a CONTIGUOUS range of units (level_wave_range): its histogram in LDS belongs to one capture at a time, and the
// wave flushes it to that capture's totals when its row changes and at its end -- with ranges, a row change is as rare as a
// capture's end, and the search for the next row starts at the previous one.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "power_export_batch.hpp" // export_row, kExportPass, kExportMaxCaptures

namespace adsb {

constexpr uint64_t kLevelPass = kExportPass; // power samples of a pass
// The captures one launch takes.  A capture's totals are kLevelWords (2053) 64-bit words, 16 424 bytes: 1024 captures are 16.04 MiB
// of device memory and as much pinned host memory, held by the handle from its first batch call on and grown to the largest
// sub-batch seen (a batch of 4096 captures goes in four launches through the same 16 MiB, where totals for all of it would be 64 MiB).
constexpr size_t kLevelBatchCaptures = 1024;

struct LevelSeg {
    uint64_t src;   // the capture's samples: uint16 real samples (16-byte aligned) / the units of the kind (aligned to the unit)
    uint64_t env;   // its envelope, one float per run of 28 power samples (4-byte aligned); 0: none
    uint64_t first; // its first unit's number; in the closing row: the number of all units
    uint64_t p_hi;  // real: the pairs it holds, n / 2 (a pair outside [0, p_hi) reads as silence)
    uint64_t m_end; // the power samples it is given: 2 (n / 4) real, n for the kinds
    uint64_t tail;  // real: the codes behind its last whole group of four that the launch counts on the rails, n % 4 -- at
                    // sample 4 (n / 4); 0 where the host counts them (adsb_level_batch_host) and for the kinds
    uint64_t tot;   // which of the launch's totals are the capture's: words [tot * kLevelWords, + kLevelWords)
};

// The units [*begin, *end) of wave w of n_waves: contiguous, in wave order, every unit exactly once, sizes differing by one at most.
// q = units / n_waves and rem = units % n_waves are the launch's (level_wave_split): a kernel has no 64-bit division to do.
ADSB_HD inline void level_wave_range(uint64_t q, uint64_t rem, uint64_t w, uint64_t *begin, uint64_t *end)
{
    *begin = w * q + (w < rem ? w : rem); // (no product of units and waves: neither is bounded by the other)
    *end = *begin + q + (w < rem ? 1 : 0);
}
inline void level_wave_split(uint64_t units, uint64_t n_waves, uint64_t *q, uint64_t *rem) { *q = units / n_waves, *rem = units % n_waves; }

// ---- host-only: building the table ----
// The table of n_captures captures into tab[0 .. rows], rows <= n_captures: capture i has m[i] power samples (and p_hi[i] pairs and
// tail[i] trailing codes; NULL for the kinds), is read at src[i] and has its envelope at env[i] (env == NULL: none has one).
// row_of[i] = the capture's row, = its totals, or UINT32_MAX where it has none.  *units = the number of all units.  Returns the rows,
// the closing one not counted.
inline uint32_t level_table(size_t n_captures, const uint64_t *m, const uint64_t *p_hi, const uint64_t *tail, const void *const *src,
                            float *const *env, LevelSeg *tab, uint32_t *row_of, uint64_t *units)
{
    uint32_t row = 0;
    uint64_t at = 0;
    for (size_t i = 0; i < n_captures; i++) {
        row_of[i] = UINT32_MAX;
        if (m[i] == 0)
            continue;
        row_of[i] = row;
        tab[row] = LevelSeg{(uint64_t)(uintptr_t)src[i], env ? (uint64_t)(uintptr_t)env[i] : 0, at, p_hi ? p_hi[i] : 0, m[i], tail ? tail[i] : 0, row};
        row++;
        at += export_units(m[i], kLevelPass);
    }
    tab[row] = LevelSeg{0, 0, at, 0, 0, 0, 0};
    *units = at;
    return row;
}

#ifdef __HIPCC__
// level_batch_kernel.hip: the n_rows captures of the table at tab_device (device memory), `units` passes in all, reduced into
// totals (n_rows x kLevelWords uint64 in device memory, zeroed by the caller on the same stream; the counts are ADDED), enqueued
// on `stream` behind the table's upload.  kind: -1 real uint16 captures, else level.h's kLevelIq16 / kLevelIq8 / kLevelPower.
// max_blocks: 0, or the most workgroups the launch may have (adsb_debug_set_level_batch_blocks).  Nothing is launched for a table
// without units.
hipError_t launch_level_batch(int kind, const LevelSeg *tab_device, uint32_t n_rows, uint64_t units, unsigned long long *totals,
                              unsigned max_blocks, hipStream_t stream);
#endif

} // namespace adsb
