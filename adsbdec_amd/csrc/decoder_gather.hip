// decoder_gather.hip -- a capture's bursts as one array (include/adsbdec_amd.h: adsb_gather_device): the capture is in device memory,
// the burst table (adsb_bursts_*) in host memory; the pieces the table names are packed into the caller's device array by ONE launch
// (gather_kernel.hip; the layout is gather.h gather_layout, adsbdec_amd/burst_archive.py layout in numpy).  Stateless as the export,
// level and burst calls are: a call changes neither the handle's stream position nor its resolver; its upload and its kernel go to
// the scan stream, behind whatever a push has left there, and the call returns when the bytes are in the caller's array.  A refusal
// launches and writes nothing.
//
// A call: the layout (refusals, offsets, the row table into the pinned half of gather_tab), one upload of the rows, the launch, the
// wait.  The table is the handle's (decoder_state.hpp: gather_tab), grown on demand; the wait at the end of a call is what makes its
// pinned half free for the next.
#include "decoder_state.hpp"
#include "gather.h"

#include <algorithm>
#include <cstring>
#include <new>
#include <vector>

using namespace adsb;

extern "C" {

uint32_t adsb_gather_chunk_words(void) { return kGatherChunk; }

long adsb_gather_device(adsb_decoder *d, const void *device_capture, size_t capture_bytes, int sample_bytes, uint64_t m, const adsb_burst *bursts,
                        size_t n_bursts, void *device_out, size_t out_cap_bytes, uint64_t *offsets)
{
    const char *what = "adsb_gather_device";
    if (!d)
        return -1;
    if (n_bursts >= 0xFFFFFFFFull)
        return d->fail("%s: n_bursts = %zu reaches 2^32 - 1", what, n_bursts);
    // the layout first, into memory of the call's own: a refusal leaves the handle's table and the caller's offsets as they were
    std::vector<uint64_t> off;
    std::vector<GatherRow> rows;
    try { // (no exception leaves a C entry point)
        off.resize(n_bursts + 1);
        rows.resize(n_bursts + 1);
    } catch (const std::bad_alloc &) {
        return d->fail("%s: out of host memory for the offsets and rows of %zu bursts", what, n_bursts);
    }
    uint64_t total = 0;
    char why[256];
    if (gather_layout(m, sample_bytes, bursts, n_bursts, off.data(), rows.data(), &total, why, sizeof why))
        return d->fail("%s: %s", what, why);
    if ((uint64_t)capture_bytes / (uint64_t)sample_bytes < m)
        return d->fail("%s: capture_bytes = %zu holds fewer than m = %llu power samples of %d bytes", what, capture_bytes, (unsigned long long)m,
                       sample_bytes);
    if (n_bursts && !device_capture)
        return d->fail("%s: NULL capture with %zu bursts to gather (burst 0 reads it first)", what, n_bursts);
    if (n_bursts && !device_out)
        return d->fail("%s: NULL output with %zu bursts to gather (burst 0 is written first)", what, n_bursts);
    if ((uintptr_t)device_capture % 16)
        return d->fail("%s: the capture's device pointer %p is not 16-byte aligned (burst 0 onward)", what, device_capture);
    if ((uintptr_t)device_out % 16)
        return d->fail("%s: the output's device pointer %p is not 16-byte aligned (burst 0 onward)", what, device_out);
    if ((uint64_t)out_cap_bytes < total) {
        size_t fit = 0;
        while (fit < n_bursts && off[fit + 1] <= (uint64_t)out_cap_bytes)
            fit++;
        return d->fail("%s: out_cap_bytes = %zu is below the %llu bytes of the %zu bursts: burst %zu is the first that does not fit", what,
                       out_cap_bytes, (unsigned long long)total, n_bursts, fit);
    }
    if (offsets)
        std::copy(off.begin(), off.end(), offsets);
    if (n_bursts == 0)
        return 0;
    HIP_TRY(d, hipSetDevice(d->device));
    const size_t tab_bytes = rows.size() * sizeof(GatherRow);
    if (d->gather_tab.reserve(tab_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return d->fail("%s: cannot allocate the %zu bytes of the %zu bursts' row table", what, tab_bytes, n_bursts);
    }
    memcpy(d->gather_tab.host.p, rows.data(), tab_bytes);
    HIP_TRY(d, hipMemcpyAsync(d->gather_tab.dev, d->gather_tab.host, tab_bytes, hipMemcpyHostToDevice, d->stream));
    HIP_TRY(d, launch_gather(device_out, device_capture, reinterpret_cast<const GatherRow *>(d->gather_tab.dev.p), (uint32_t)n_bursts, total / 16,
                             d->stream));
    WAIT_STREAM(d, d->stream, "the scan stream");
    return (long)total;
}

} // extern "C"
