// decoder_flavour.hip -- the part of flavour.hpp that speaks through the handle: the judgement of a format number (the only
// sentences a flavour supplies) and what every _iq and _power call asks of its samples, stream pushes included.
#include "decoder_state.hpp"
#include "level.h"

using namespace adsb;

static_assert(kLevelKindIq16 == kLevelIq16 && kLevelKindIq8 == kLevelIq8 && kLevelKindPower == kLevelPower, "flavour.hpp restates the level kinds of level.h");

namespace adsb {

// What every _as call checks first: the format.  0: converted (*elem bytes per sample); 1: the uint16 code itself; -1: refused.
int format_dispatch(adsb_decoder *d, const char *what, int fmt, size_t *elem)
{
    *elem = format_element_bytes(fmt);
    if (*elem)
        return 0;
    if (fmt == kFmtUint16Real || fmt == kFmtRaw)
        return 1;
    if (fmt == 0 || fmt == 2)
        return d->fail("%s: format %d (%s) is not a real format: libairspy has already mixed, filtered and decimated an IQ stream, so it has no "
                       "raw twin to be decoded as", what, fmt, fmt == 0 ? "FLOAT32_IQ" : "INT16_IQ");
    return d->fail("%s: unknown sample format %d (1 FLOAT32_REAL, 3 INT16_REAL, 4 UINT16_REAL, 5 RAW)", what, fmt);
}

int flavour_as(adsb_decoder *d, const char *what, int fmt, Flavour *f)
{
    size_t elem;
    const int k = format_dispatch(d, what, fmt, &elem);
    if (k == 0)
        *f = flavour_converted(fmt);
    return k;
}

int flavour_iq(adsb_decoder *d, const char *what, int fmt, Flavour *f)
{
    if (!iq_sample_bytes(fmt))
        return d->fail("%s: format %d is not an IQ format (0 FLOAT32_IQ, 2 INT16_IQ, 8 INT8_IQ; real samples go through the _as calls)", what, fmt);
    *f = flavour_of_iq(fmt);
    return 0;
}

// ---- complex samples and float32 power samples (the _iq and _power calls; include/adsbdec_amd.h) ----
// What every such call checks of n samples at p before anything of the handle changes; the stream is at at_units.  n counts complex
// or power samples; the stream counts 16-bit units, two per sample, so everything behind these checks is the uint16 machinery with
// 2 n -- for a power sample, 4 bytes as a complex int16 sample is, INT16_IQ's road: copies, staging, compaction, in-place scans, the
// EOF rule and the count pass.  An int8 stream (fmt 8) counts bytes, two per complex sample as well: the same machinery with the same
// 2 n, and a unit of one byte where it copies.
int units_refusal(adsb_decoder *d, const char *what, const Flavour &F, const void *p, size_t n, uint64_t at_units)
{
    const bool power = F.kind == kKindPower;
    if ((uint64_t)n >= (1ull << 31) || at_units + 2 * (uint64_t)n >= (1ull << 32))
        return d->fail("%s: the stream would reach 2^31 %s samples (%llu + %zu): %s streams end below", what, power ? "power" : "complex",
                       (unsigned long long)(at_units / 2), n, power ? "power" : "IQ");
    if (n && !p)
        return d->fail("%s: NULL samples", what);
    if (F.in_align && (uintptr_t)p % F.in_align != 0)
        return d->fail("%s: device pointer %p is not %u-byte aligned", what, p, F.in_align);
    return 0;
}

int iq_refusal(adsb_decoder *d, const char *what, int fmt, const void *p, size_t n, bool device, uint64_t at_units)
{
    Flavour f;
    return flavour_iq(d, what, fmt, &f) ? -1 : units_refusal(d, what, device ? f : f.on_host(), p, n, at_units);
}

int power_refusal(adsb_decoder *d, const char *what, const void *p, size_t n, bool device, uint64_t at_units)
{
    return units_refusal(d, what, device ? flavour_power() : flavour_power().on_host(), p, n, at_units);
}

} // namespace adsb
