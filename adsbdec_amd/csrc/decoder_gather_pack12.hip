// decoder_gather_pack12.hip -- a real capture's bursts as one array of packed 12-bit samples (include/adsbdec_amd.h:
// adsb_gather_pack12_device, _as, _packed): the capture is in device memory, the burst table (adsb_bursts_*) in host memory; the pieces
// the table names are packed into the caller's device array by ONE launch (gather_pack12_kernel.hip; the layout is gather_pack12.h
// gather_pack12_layout, adsbdec_amd/burst_archive.py layout12 / gather12 in numpy).  Every flavour gathers from a uint16 twin in HBM:
// a uint16 capture is its own; an _as (fmt 1 | 3) or _packed capture is first converted or unpacked, by the launch and into the scratch
// that adsb_decode_device_as / _packed use (decoder_stage.hip to_scratch), on the same stream.  Stateless as adsb_gather_device is: a
// call changes neither the handle's stream position nor its resolver, and returns when the bytes are in the caller's array.  A refusal
// launches, writes and counts nothing -- the checks all stand in front of the conversion.
#include "decoder_state.hpp"
#include "gather_pack12.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

using namespace adsb;

namespace {

// What a call has checked and laid out, before anything is enqueued.
struct Pack12Plan {
    std::vector<uint64_t> off;
    std::vector<GatherPack12Row> rows;
    uint64_t total = 0;
};

// The checks every flavour shares, and the layout.  in_align: the flavour's (flavour.hpp).
int pack12_plan(adsb_decoder *d, const char *what, const void *device_in, unsigned in_align, size_t n, const adsb_burst *bursts, size_t n_bursts,
                const void *device_out, size_t out_cap_bytes, Pack12Plan &p)
{
    if (n_bursts >= 0xFFFFFFFFull)
        return d->fail("%s: n_bursts = %zu reaches 2^32 - 1", what, n_bursts);
    if ((uint64_t)n >= (1ull << 32))
        return d->fail("%s: n = %zu samples reaches 2^32 (burst 0 onward: no real capture a call decodes is that long)", what, n);
    try { // (no exception leaves a C entry point)
        p.off.resize(n_bursts + 1);
        p.rows.resize(n_bursts + 1);
    } catch (const std::bad_alloc &) {
        return d->fail("%s: out of host memory for the offsets and rows of %zu bursts", what, n_bursts);
    }
    char why[256];
    if (gather_pack12_layout(power_samples_produced(n), bursts, n_bursts, p.off.data(), p.rows.data(), &p.total, why, sizeof why))
        return d->fail("%s: %s", what, why);
    if (n_bursts && !device_in)
        return d->fail("%s: NULL capture with %zu bursts to gather (burst 0 reads it first)", what, n_bursts);
    if (n_bursts && !device_out)
        return d->fail("%s: NULL output with %zu bursts to gather (burst 0 is written first)", what, n_bursts);
    if ((uintptr_t)device_in % in_align)
        return d->fail("%s: the capture's device pointer %p is not %u-byte aligned (burst 0 onward)", what, device_in, in_align);
    if ((uintptr_t)device_out % 16)
        return d->fail("%s: the output's device pointer %p is not 16-byte aligned (burst 0 onward)", what, device_out);
    if ((uint64_t)out_cap_bytes < p.total) {
        size_t fit = 0;
        while (fit < n_bursts && p.off[fit + 1] <= (uint64_t)out_cap_bytes)
            fit++;
        return d->fail("%s: out_cap_bytes = %zu is below the %llu bytes of the %zu bursts: burst %zu is the first that does not fit", what,
                       out_cap_bytes, (unsigned long long)p.total, n_bursts, fit);
    }
    return 0;
}

// The rows up, the counter zeroed, the launch, the counter back, the wait: on the scan stream, behind what made `u16`.
long pack12_run(adsb_decoder *d, const char *what, const uint16_t *u16, const Pack12Plan &p, size_t n_bursts, void *device_out, uint64_t *over)
{
    HIP_TRY(d, hipSetDevice(d->device));
    const size_t tab_bytes = p.rows.size() * sizeof(GatherPack12Row);
    if (d->gather_tab.reserve(tab_bytes) != hipSuccess || d->gather_over.reserve(1) != hipSuccess) {
        (void)hipGetLastError();
        return d->fail("%s: cannot allocate the %zu bytes of the %zu bursts' row table", what, tab_bytes, n_bursts);
    }
    memcpy(d->gather_tab.host.p, p.rows.data(), tab_bytes);
    HIP_TRY(d, hipMemcpyAsync(d->gather_tab.dev, d->gather_tab.host, tab_bytes, hipMemcpyHostToDevice, d->stream));
    HIP_TRY(d, hipMemsetAsync(d->gather_over.dev, 0, sizeof(unsigned long long), d->stream));
    HIP_TRY(d, launch_gather_pack12(device_out, u16, reinterpret_cast<const GatherPack12Row *>(d->gather_tab.dev.p), (uint32_t)n_bursts,
#if ADSB_GATHER_PACK12_LANE3
                                    p.rows.back().t_first,
#else
                                    p.total / 16,
#endif
                                    d->gather_over.dev, d->stream));
    HIP_TRY(d, hipMemcpyAsync(d->gather_over.host, d->gather_over.dev, sizeof(unsigned long long), hipMemcpyDeviceToHost, d->stream));
    WAIT_STREAM(d, d->stream, "the scan stream");
    if (over)
        *over = d->gather_over.host.p[0];
    return (long)p.total;
}

// behind the checks: what a call without work returns, the caller's offsets filled either way
bool pack12_done_early(const Pack12Plan &p, size_t n_bursts, uint64_t *offsets, uint64_t *over)
{
    if (offsets)
        std::copy(p.off.begin(), p.off.end(), offsets);
    if (n_bursts)
        return false;
    if (over)
        *over = 0;
    return true;
}

// One call over its flavour F: the checks and the layout, what F puts in front (decoder_stage.hip: a table with a burst has a power
// sample to read), the launch behind it on the same stream.
long gather_pack12(adsb_decoder *d, const char *what, const Flavour &F, const void *device_in, size_t n, const adsb_burst *bursts, size_t n_bursts,
                   void *device_out, size_t out_cap_bytes, uint64_t *offsets, uint64_t *over)
{
    if (F.groups8 && n % kPackedGroupSamples)
        return d->fail("%s: n = %zu is not a multiple of 8 (packed samples come in groups of 8 in 12 bytes; burst 0 onward)", what, n);
    Pack12Plan p;
    if (pack12_plan(d, what, device_in, F.in_align, n, bursts, n_bursts, device_out, out_cap_bytes, p))
        return -1;
    if (pack12_done_early(p, n_bursts, offsets, over))
        return 0;
    const void *u16 = flavour_to_scratch(d, what, F, device_in, n);
    return u16 ? pack12_run(d, what, static_cast<const uint16_t *>(u16), p, n_bursts, device_out, over) : -1;
}

} // namespace

extern "C" {

long adsb_gather_pack12_device(adsb_decoder *d, const void *device_samples, size_t n, const adsb_burst *bursts, size_t n_bursts, void *device_out,
                               size_t out_cap_bytes, uint64_t *offsets, uint64_t *over)
{
    return d ? gather_pack12(d, "adsb_gather_pack12_device", flavour_uint16(), device_samples, n, bursts, n_bursts, device_out, out_cap_bytes, offsets, over)
             : -1;
}

long adsb_gather_pack12_device_as(adsb_decoder *d, int fmt, const void *device_samples, size_t n, const adsb_burst *bursts, size_t n_bursts,
                                  void *device_out, size_t out_cap_bytes, uint64_t *offsets, uint64_t *over)
{
    const char *what = "adsb_gather_pack12_device_as";
    if (!d)
        return -1;
    if (!format_element_bytes(fmt)) // (this call forwards nothing: its sentence, not flavour_as's)
        return d->fail("%s: format %d is none of 1 (FLOAT32_REAL), 3 (INT16_REAL): a uint16 capture goes to adsb_gather_pack12_device (burst 0 onward)",
                       what, fmt);
    // (16 bytes, not the element's size as the other _as calls ask)
    return gather_pack12(d, what, flavour_converted(fmt).at(16), device_samples, n, bursts, n_bursts, device_out, out_cap_bytes, offsets, over);
}

long adsb_gather_pack12_device_packed(adsb_decoder *d, const void *device_packed, size_t n, const adsb_burst *bursts, size_t n_bursts,
                                      void *device_out, size_t out_cap_bytes, uint64_t *offsets, uint64_t *over)
{
    return d ? gather_pack12(d, "adsb_gather_pack12_device_packed", flavour_packed(), device_packed, n, bursts, n_bursts, device_out, out_cap_bytes,
                             offsets, over)
             : -1;
}

} // extern "C"
