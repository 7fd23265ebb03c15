// decoder_bursts.hip -- the gate behind the envelope (include/adsbdec_amd.h: adsb_bursts_*): the envelope a level call wrote, or any
// float array of the caller's, -> the ordered table of its bursts (burst_kernel.hip; the definition is adsbdec_amd/levels.py bursts).
// Stateless as the level and export calls are: a call changes neither the handle's stream position nor its resolver; its kernels go
// to the scan stream, behind whatever a push has left there, and the call returns when the table is in the caller's memory.  A
// refusal launches and writes nothing.
//
// A call: the summaries and the combine (burst.h launch_burst_count), B back to the host, and -- where there is a burst and room
// for one -- a memset of min(B, cap) records, the emit and the copy of those records.  The scratch is the handle's
// (decoder_state.hpp: burst_scratch, burst_total, burst_tab), grown on demand.
#include "decoder_state.hpp"
#include "burst.h"

#include <cmath>

using namespace adsb;

namespace {

static_assert(sizeof(adsb_burst) == 4 * sizeof(uint32_t), "burst.h: a record is four words");
constexpr uint32_t kBurstRunLimit = 1u << 30; // the most lead or hang may be

int bursts_refusal(adsb_decoder *d, const char *what, const char *where, const float *env, size_t n_env, float threshold, uint32_t lead,
                   uint32_t hang, const adsb_burst *bursts, size_t cap)
{
    uint32_t tb;
    memcpy(&tb, &threshold, sizeof tb);
    if (!env && n_env)
        return d->fail("%s: NULL envelope with n_env = %zu", what, n_env);
    if ((uintptr_t)env % 4)
        return d->fail("%s: %s pointer %p is not 4-byte aligned", what, where, (const void *)env);
    if (n_env >= (1ull << 31))
        return d->fail("%s: n_env = %zu reaches 2^31 runs", what, n_env);
    if (std::isnan(threshold) || tb >> 31)
        return d->fail("%s: the threshold (bits 0x%08x) must be a float with the sign bit clear, and no NaN", what, tb);
    if (lead > kBurstRunLimit || hang > kBurstRunLimit)
        return d->fail("%s: lead = %u and hang = %u may be 2^30 runs at most", what, lead, hang);
    if (!bursts && cap)
        return d->fail("%s: NULL table with cap = %zu (to count only: NULL and 0)", what, cap);
    return 0;
}

// checked by the caller; n_env > 0
long bursts_run(adsb_decoder *d, const char *what, const float *device_env, size_t n_env, float threshold, uint32_t lead, uint32_t hang,
                adsb_burst *bursts, size_t cap)
{
    HIP_TRY(d, hipSetDevice(d->device));
    BurstArgs a{};
    a.pad = (uint32_t)((uintptr_t)device_env % 16 / 4);
    a.base = device_env - a.pad;
    a.runs = (uint32_t)n_env;
    memcpy(&a.threshold_bits, &threshold, sizeof a.threshold_bits);
    a.lead = lead, a.hang = hang, a.join = lead + hang + 1;
    a.n_tiles = burst_tiles(n_env, a.pad);
    if (d->burst_scratch.reserve((size_t)2 * kBurstTileWords * a.n_tiles) != hipSuccess || d->burst_total.reserve(1) != hipSuccess) {
        (void)hipGetLastError();
        return d->fail("%s: cannot allocate the %u tiles' %zu bytes on the device", what, a.n_tiles,
                       (size_t)2 * kBurstTileWords * a.n_tiles * sizeof(uint32_t));
    }
    a.summaries = d->burst_scratch;
    a.rows = d->burst_scratch + (size_t)kBurstTileWords * a.n_tiles;
    a.total = d->burst_total.dev;
    HIP_TRY(d, launch_burst_count(a, d->stream));
    HIP_TRY(d, hipMemcpyAsync(d->burst_total.host, d->burst_total.dev, sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
    WAIT_STREAM(d, d->stream, "the scan stream");
    const uint32_t total = d->burst_total.host[0];
    const size_t n_out = std::min<size_t>(total, cap);
    if (n_out == 0)
        return (long)total;
    if (d->burst_tab.reserve(4 * n_out) != hipSuccess) {
        (void)hipGetLastError();
        return d->fail("%s: cannot allocate a table of %zu bursts on the device", what, n_out);
    }
    a.table = d->burst_tab;
    a.cap = (uint32_t)n_out;
    HIP_TRY(d, hipMemsetAsync(d->burst_tab, 0, n_out * sizeof(adsb_burst), d->stream));
    HIP_TRY(d, launch_burst_emit(a, d->stream));
    HIP_TRY(d, hipMemcpyAsync(bursts, d->burst_tab, n_out * sizeof(adsb_burst), hipMemcpyDeviceToHost, d->stream));
    WAIT_STREAM(d, d->stream, "the scan stream");
    return (long)total;
}

} // namespace

extern "C" {

uint32_t adsb_burst_tile_runs(void) { return kBurstTileRuns; }

long adsb_bursts_device(adsb_decoder *d, const float *device_env, size_t n_env, float threshold, uint32_t lead, uint32_t hang,
                        adsb_burst *bursts, size_t cap)
{
    const char *what = "adsb_bursts_device";
    if (!d)
        return -1;
    if (bursts_refusal(d, what, "device", device_env, n_env, threshold, lead, hang, bursts, cap))
        return -1;
    if (n_env == 0)
        return 0;
    return bursts_run(d, what, device_env, n_env, threshold, lead, hang, bursts, cap);
}

long adsb_bursts_host(adsb_decoder *d, const float *env, size_t n_env, float threshold, uint32_t lead, uint32_t hang, adsb_burst *bursts,
                      size_t cap)
{
    const char *what = "adsb_bursts_host";
    if (!d)
        return -1;
    if (bursts_refusal(d, what, "host", env, n_env, threshold, lead, hang, bursts, cap))
        return -1;
    if (n_env == 0)
        return 0;
    HIP_TRY(d, hipSetDevice(d->device));
    if (d->pow_buf.reserve((n_env + 65535) & ~(size_t)65535) != hipSuccess) {
        (void)hipGetLastError();
        return d->fail("%s: cannot allocate the envelope's %zu bytes on the device", what, n_env * sizeof(float));
    }
    HIP_TRY(d, hipMemcpyAsync(d->pow_buf, env, n_env * sizeof(float), hipMemcpyHostToDevice, d->copy_stream[0]));
    WAIT_STREAM(d, d->copy_stream[0], "a copy stream");
    return bursts_run(d, what, d->pow_buf, n_env, threshold, lead, hang, bursts, cap);
}

} // extern "C"
