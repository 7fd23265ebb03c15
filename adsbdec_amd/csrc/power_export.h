// power_export.h -- the launches of power_export_kernel.hip: the front end's float32 power samples written out instead of being
// turned into sign planes (include/adsbdec_amd.h: the adsb_power_* calls; decoder_export.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#pragma GCC visibility push(hidden)

namespace adsb {

// out[m - m_begin] = power sample m of the stream for m in [m_begin, m_end), from the uint16 real samples of pairs [p_lo, p_hi)
// (x[0] is pair pbuf0; 16-byte aligned at a multiple of 4 pairs).  m_begin % 28 == 0; out 16-byte aligned; a pair outside
// [p_lo, p_hi) reads as (0x800, 0x800).  Nothing is launched for an empty window.
hipError_t launch_power_export(const uint32_t *x, int64_t pbuf0, int64_t p_lo, int64_t p_hi, int64_t m_begin, int64_t m_end, float *out,
                               hipStream_t stream);
// out[m] = iq_power(sample m) for the n complex int16 samples at x (4-byte aligned); out 16-byte aligned
hipError_t launch_iq_power_export(const uint32_t *x, size_t n, float *out, hipStream_t stream);

} // namespace adsb

#pragma GCC visibility pop
