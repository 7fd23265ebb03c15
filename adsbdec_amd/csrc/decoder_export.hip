// decoder_export.hip -- the export calls (include/adsbdec_amd.h: adsb_power_*): the front end's float32 power samples, the
// reference's ampbuff (air.c:54-91), written to an array of the caller's instead of being scanned.  Stateless like the shard scans
// beside them (decoder_shard.hip): a call changes neither the handle's stream position nor its resolver; its kernel goes to the
// scan stream, behind whatever a push has left there, and the call returns when the floats are written.  (The handle: decoder_state.hpp.)
#include "decoder_state.hpp"
#include "power_export.h"

using namespace adsb;

namespace {

// What the window call asks of its window, before anything is launched.
int export_window_refusal(adsb_decoder *d, const char *what, uint64_t first_sample, size_t n, uint64_t m_begin, uint64_t m_end,
                          size_t power_cap)
{
    if (shard_too_long(d, what, first_sample, n, 0)) // (on a long-stream handle too: the counter wrap's ring jump is adsb_seam_power's)
        return -1;
    if (first_sample % 8)
        return d->fail("%s: buffer must start at a multiple of 8 samples", what);
    if (m_begin % 28)
        return d->fail("%s: m_begin must be a multiple of 28", what);
    if (m_end < m_begin)
        return d->fail("%s: m_end %llu lies below m_begin %llu", what, (unsigned long long)m_end, (unsigned long long)m_begin);
    if (m_begin > (1ull << 31) || m_end > (1ull << 31) || 2 * m_begin < first_sample || 2 * m_end > first_sample + n)
        return d->fail("%s: the buffer does not hold the own pair of every power sample of the window (2 m_begin >= first_sample and "
                       "2 m_end <= first_sample + n)", what);
    if (m_end - m_begin > power_cap)
        return d->fail("%s: the window has %llu power samples, the array holds %zu", what, (unsigned long long)(m_end - m_begin), power_cap);
    return 0;
}

int export_pointer_refusal(adsb_decoder *d, const char *what, const void *device_samples, const float *device_power, bool empty)
{
    if ((uintptr_t)device_samples % 16)
        return d->fail("%s: buffer must start 16-byte aligned (%p)", what, device_samples);
    if ((uintptr_t)device_power % 16)
        return d->fail("%s: the power array must be 16-byte aligned (%p)", what, (const void *)device_power);
    if (!empty && (!device_samples || !device_power))
        return d->fail("%s: NULL buffer", what);
    return 0;
}

// the launch of a checked window, and the wait for it
long export_window(adsb_decoder *d, const void *device_samples, uint64_t first_sample, size_t n, uint64_t m_begin, uint64_t m_end,
                   float *device_power)
{
    if (m_end == m_begin)
        return 0;
    HIP_TRY(d, hipSetDevice(d->device));
    const int64_t p0 = (int64_t)(first_sample / 2);
    HIP_TRY(d, launch_power_export(static_cast<const uint32_t *>(device_samples), p0, p0, (int64_t)((first_sample + n) / 2), (int64_t)m_begin,
                                   (int64_t)m_end, device_power, d->stream));
    WAIT_STREAM(d, d->stream, "the scan stream");
    return (long)(m_end - m_begin);
}

// A whole real capture of the flavour F in HBM as a fresh stream.  A uint16 capture is read where it lies: its pointers are checked
// first, in the window call's words; a packed or converted one is read by the launch in front (decoder_stage.hip), on the same stream.
long export_capture(adsb_decoder *d, const char *what, const Flavour &F, const void *device_samples, size_t n, float *device_power, size_t power_cap)
{
    const bool own = F.front == Flavour::kNone;
    const uint64_t m_end = F.power_samples(n);
    if (F.groups8 && n % kPackedGroupSamples)
        return d->fail("%s: n = %zu is not a multiple of 8 (packed samples come in groups of 8 in 12 bytes)", what, n);
    if (own) {
        if (export_pointer_refusal(d, what, device_samples, device_power, m_end == 0))
            return -1;
    } else if ((uintptr_t)device_samples % F.in_align)
        return d->fail("%s: device pointer %p is not %zu-byte aligned", what, device_samples, (size_t)F.in_align);
    if (export_window_refusal(d, what, 0, n, 0, m_end, power_cap) || (!own && export_pointer_refusal(d, what, nullptr, device_power, true)))
        return -1;
    if (m_end == 0)
        return 0;
    if (!device_samples || !device_power)
        return d->fail("%s: NULL buffer", what);
    const void *u16 = flavour_to_scratch(d, what, F, device_samples, n);
    return u16 ? export_window(d, u16, 0, n, 0, m_end, device_power) : -1;
}

} // namespace

extern "C" {

long adsb_power_window(adsb_decoder *d, const void *device_samples, uint64_t first_sample, size_t n, uint64_t m_begin, uint64_t m_end,
                       float *device_power, size_t power_cap)
{
    const char *what = "adsb_power_window";
    if (!d)
        return -1;
    if (export_window_refusal(d, what, first_sample, n, m_begin, m_end, power_cap) ||
        export_pointer_refusal(d, what, device_samples, device_power, m_end == m_begin))
        return -1;
    return export_window(d, device_samples, first_sample, n, m_begin, m_end, device_power);
}

long adsb_power_window_host(adsb_decoder *d, const uint16_t *samples, uint64_t first_sample, size_t n, uint64_t m_begin, uint64_t m_end,
                            float *power, size_t power_cap)
{
    const char *what = "adsb_power_window_host";
    if (!d)
        return -1;
    if (export_window_refusal(d, what, first_sample, n, m_begin, m_end, power_cap))
        return -1;
    if (m_end == m_begin)
        return 0;
    if (!samples || !power)
        return d->fail("%s: NULL buffer", what);
    const size_t count = (size_t)(m_end - m_begin);
    if (window_in(d, samples, n, count) || export_window(d, d->win_buf, first_sample, n, m_begin, m_end, d->pow_buf) < 0 ||
        floats_out(d, power, count))
        return -1;
    return (long)count;
}

long adsb_power_device(adsb_decoder *d, const void *device_samples, size_t n, float *device_power, size_t power_cap)
{
    return d ? export_capture(d, "adsb_power_device", flavour_uint16(), device_samples, n, device_power, power_cap) : -1;
}

long adsb_power_device_as(adsb_decoder *d, int fmt, const void *device_samples, size_t n, float *device_power, size_t power_cap)
{
    const char *what = "adsb_power_device_as";
    Flavour F;
    if (!d)
        return -1;
    const int k = flavour_as(d, what, fmt, &F);
    if (k < 0)
        return -1;
    if (k)
        return adsb_power_device(d, device_samples, n, device_power, power_cap);
    return export_capture(d, what, F, device_samples, n, device_power, power_cap);
}

long adsb_power_device_packed(adsb_decoder *d, const void *device_packed, size_t n, float *device_power, size_t power_cap)
{
    return d ? export_capture(d, "adsb_power_device_packed", flavour_packed(), device_packed, n, device_power, power_cap) : -1;
}

long adsb_power_device_iq(adsb_decoder *d, int fmt, const void *device_samples, size_t n, float *device_power, size_t power_cap)
{
    const char *what = "adsb_power_device_iq";
    if (!d)
        return -1;
    if (fmt == kFmtInt8Iq) // (decoded, not exported: an int8 sample's power is 256 (I^2 + Q^2), which a caller has in one line)
        return d->fail("%s: format 8 (INT8_IQ) is not exported: the power export takes fmt 0 FLOAT32_IQ and 2 INT16_IQ only", what);
    if (iq_refusal(d, what, fmt, device_samples, n, true, 0))
        return -1;
    if ((uintptr_t)device_power % 16)
        return d->fail("%s: the power array must be 16-byte aligned (%p)", what, (const void *)device_power);
    if (n > power_cap)
        return d->fail("%s: the capture has %zu power samples, the array holds %zu", what, n, power_cap);
    if (n == 0)
        return 0;
    if (!device_power)
        return d->fail("%s: NULL buffer", what);
    HIP_TRY(d, hipSetDevice(d->device));
    // (FLOAT32_IQ: to the int16 grid first, by the conversion the _iq pushes use and into their scratch)
    const void *iq16 = flavour_to_scratch(d, what, flavour_of_iq(fmt), device_samples, n);
    if (!iq16)
        return -1;
    HIP_TRY(d, launch_iq_power_export(static_cast<const uint32_t *>(iq16), n, device_power, d->stream));
    WAIT_STREAM(d, d->stream, "the scan stream");
    return (long)n;
}

} // extern "C"
