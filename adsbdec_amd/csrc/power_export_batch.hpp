// power_export_batch.hpp -- the table of power_export_batch_kernel.hip (include/adsbdec_amd.h: the adsb_power_batch_* calls): the
// scheme of packed12.h's Unpack12Seg, over the export's units of work.  Host + device code: the row search is the kernels' and the
// CPU test's (tests/cpp/power_export_batch_rows.cpp); building the table is host-only.
//
// The units of all captures are numbered in ONE space, capture after capture.  A unit of the real export is a PASS -- one wave, 64
// runs, 1792 power samples of ONE capture: a capture of m power samples owns ceil(m / 1792) consecutive pass numbers, and a pass
// never spans two captures.  A unit of the IQ export is a GROUP of four complex samples, ceil(n / 4) per capture, the last one
// possibly short.  A row per capture THAT HAS UNITS, in capture order (a capture without power samples has no row and costs
// nothing); the row behind the last one holds the total.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "scan_kernel_format.h" // ADSB_HD

namespace adsb {

constexpr uint64_t kExportPass = 64 * 28;   // power samples of a pass (power_export_batch_kernel.hip holds it to 64 * kRun)
constexpr uint64_t kExportIqGroup = 4;      // complex samples of a group
constexpr unsigned kExportIqChunk = 256;    // consecutive groups a block looks its rows up for at once (= its lanes)
constexpr uint64_t kExportMaxCaptures = 0xFFFFFFFEull; // rows are indexed in 32 bits, and one more closes the table

struct ExportSeg {
    uint64_t src;   // the capture's samples: uint16 real samples (16-byte aligned) / int16 complex samples (4-byte aligned)
    uint64_t out;   // its float32 power samples (16-byte aligned)
    uint64_t first; // its first unit's number; in the closing row: the number of all units
    uint64_t p_hi;  // real: the pairs it holds, n / 2 (a pair outside [0, p_hi) reads as silence)
    uint64_t m_end; // the power samples it is given: 2 (n / 4) real, n IQ
};

// The last row of tab[lo .. hi] whose first unit is <= u (tab[lo].first <= u is the caller's).  Tab: a pointer to ExportSeg in
// whatever address space the caller holds the table in.
template <class Tab> ADSB_HD inline uint32_t export_row(Tab tab, uint32_t lo, uint32_t hi, uint64_t u)
{
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (tab[mid].first <= u)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// ---- host-only: building the table ----
// units of a capture that is given m power samples
inline uint64_t export_units(uint64_t m, uint64_t per_unit) { return (m + per_unit - 1) / per_unit; }

// The table of n_captures captures into tab[0 .. rows], rows <= n_captures: capture i has m[i] power samples (and p_hi[i] pairs; NULL
// for IQ captures), is read at src[i] and written at out[i].  *units = the number of all units.  Returns the rows, the closing
// one not counted.
inline uint32_t export_table(size_t n_captures, const uint64_t *m, const uint64_t *p_hi, const void *const *src, float *const *out,
                             uint64_t per_unit, ExportSeg *tab, uint64_t *units)
{
    uint32_t row = 0;
    uint64_t at = 0;
    for (size_t i = 0; i < n_captures; i++) {
        if (m[i] == 0)
            continue;
        tab[row++] = ExportSeg{(uint64_t)(uintptr_t)src[i], (uint64_t)(uintptr_t)out[i], at, p_hi ? p_hi[i] : 0, m[i]};
        at += export_units(m[i], per_unit);
    }
    tab[row] = ExportSeg{0, 0, at, 0, 0};
    *units = at;
    return row;
}

#ifdef __HIPCC__
// power_export_batch_kernel.hip: the n_rows captures of the table at tab_device (device memory), `units` passes / groups in all,
// enqueued on `stream` behind the table's upload.  Nothing is launched for a table without units.
hipError_t launch_power_export_batch(const ExportSeg *tab_device, uint32_t n_rows, uint64_t units, hipStream_t stream);
hipError_t launch_iq_power_export_batch(const ExportSeg *tab_device, uint32_t n_rows, uint64_t units, hipStream_t stream);
#endif

} // namespace adsb
