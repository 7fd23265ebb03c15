// level.h -- the launches of level_kernel.hip: the level report of a capture's power samples (include/adsbdec_amd.h: the
// adsb_level_* calls; decoder_level.hip).  The front ends of the export (power_export.h) with a reduction where its stores are.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "scan_kernel.h" // kRun

#pragma GCC visibility push(hidden)

namespace adsb {

// floats of the envelope of m power samples: one per run (host-only)
inline size_t env_floats(uint64_t m) { return (size_t)((m + kRun - 1) / kRun); }

constexpr int kLevelBins = 2048;                // bin = bits >> 20 of a sign-clear float: 8 per octave
constexpr int kLevelWords = 5 + kLevelBins;      // adsb_level_report as uint64 words: samples, negative, rail_lo, rail_hi, over, hist[]
constexpr int kLevelRowWords = 4 + kLevelBins;   // a workgroup's row of 32-bit counts (measurement builds with ADSB_LEVEL_FLUSH=1)
// what a launch may be given of the handle's: the workgroups a level launch has at most, and with them the rows
unsigned level_max_blocks();
bool level_uses_rows();

// The kinds the element-wise kernel reads: a unit IS a power sample.
constexpr int kLevelIq16 = 0, kLevelIq8 = 1, kLevelPower = 2;

// The power samples [0, m_end) of the real capture at x (pairs [0, p_hi), 16-byte aligned; a fresh stream: the pairs before it
// read as silence), reduced: totals (kLevelWords uint64 in device memory, zeroed by the caller on the same stream) gets the
// counts ADDED, env (NULL: none) one float per 28 power samples.  rows: kLevelRowWords x level_max_blocks() uint32 where
// level_uses_rows(), else unused.  Nothing is launched for m_end == 0.
hipError_t launch_level(const uint32_t *x, int64_t p_hi, int64_t m_end, unsigned long long *totals, float *env, uint32_t *rows,
                        hipStream_t stream);
// ... of the n units at x: complex int16 samples (4-byte aligned), complex int8 samples (2-byte aligned), float32 power samples
// (4-byte aligned)
hipError_t launch_level_units(int kind, const void *x, size_t n, unsigned long long *totals, float *env, uint32_t *rows, hipStream_t stream);

} // namespace adsb

#pragma GCC visibility pop
