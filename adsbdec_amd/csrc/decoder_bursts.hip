// decoder_bursts.hip -- the gate behind the envelope (include/adsbdec_amd.h: adsb_bursts_*): the envelope a level call wrote, or any
// float array of the caller's, -> the ordered table of its bursts (burst_kernel.hip; the definition is adsbdec_amd/levels.py bursts).
// Stateless as the level and export calls are: a call changes neither the handle's stream position nor its resolver; its kernels go
// to the scan stream, behind whatever a push has left there, and the call returns when the table is in the caller's memory.  A
// refusal launches and writes nothing.
//
// A call: the summaries and the combine (burst.h launch_burst_count), B back to the host, and -- where there is a burst and room
// for one -- a memset of min(B, cap) records, the emit and the copy of those records.  The scratch is the handle's
// (decoder_state.hpp: burst_scratch, burst_total, burst_tab), grown on demand.
//
// adsb_bursts_slice_*: the same for a SLICE of a stream (burst_slice_kernel.hip; the definition is levels.py bursts_slice), with the
// same launches, scratch and stream.  The kernels count the cluster that earlier slices left open as burst 0 and write every record
// in stream runs; the last burst comes back behind the records, with its true first and last hot run.  The host's part is two
// records: what the carried cluster had before this slice goes into burst 0, and the last burst goes into the table where it is
// closed (final, or last + join < the runs seen: no run that could still join it is to come) and into the carry where it is not.
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

int bursts_slice_refusal(adsb_decoder *d, const char *what, size_t n_env, const adsb_burst_carry *in, const adsb_burst_carry *out)
{
    if (!in || !out)
        return d->fail("%s: NULL carry (in = %p, out = %p)", what, (const void *)in, (const void *)out);
    if (in->runs + n_env >= (1ull << 31)) // (n_env < 2^31: checked before)
        return d->fail("%s: the stream would reach 2^31 runs (%llu covered, n_env = %zu)", what, (unsigned long long)in->runs, n_env);
    if (in->open && !(in->first <= in->last && in->last < in->runs && in->hot >= 1))
        return d->fail("%s: the open carry is not first <= last < runs with hot >= 1 (first = %u, last = %u, runs = %llu, hot = %u)", what,
                       in->first, in->last, (unsigned long long)in->runs, in->hot);
    return 0;
}

uint32_t float_bits(float f)
{
    uint32_t b;
    memcpy(&b, &f, sizeof b);
    return b;
}

float larger_bits(float p, float q) { return float_bits(p) > float_bits(q) ? p : q; }

// checked by the caller; c: the carry in, a copy (in may be out); n_env may be 0: nothing is launched then
long bursts_slice_run(adsb_decoder *d, const char *what, const float *device_env, size_t n_env, float threshold, uint32_t lead,
                      uint32_t hang, const adsb_burst_carry c, int final, adsb_burst *bursts, size_t cap, adsb_burst_carry *out)
{
    const uint64_t seen = c.runs + n_env, join = (uint64_t)lead + hang + 1;
    uint32_t total = c.open ? 1 : 0;             // the clusters of this call, the carried one included
    adsb_burst last{c.first, c.last + 1, 0, 0};  // the last of them as the emit leaves it: {first hot run, last hot run + 1, hot, peak}
    size_t n_out = 0;
    if (n_env) {
        HIP_TRY(d, hipSetDevice(d->device));
        BurstArgs a{};
        a.pad = (uint32_t)((uintptr_t)device_env % 16 / 4);
        a.base = device_env - a.pad;
        a.runs = (uint32_t)n_env;
        memcpy(&a.threshold_bits, &threshold, sizeof a.threshold_bits);
        a.lead = lead, a.hang = hang, a.join = (uint32_t)join;
        a.n_tiles = burst_tiles(n_env, a.pad);
        const BurstSlice sl{(uint32_t)c.runs, c.open ? c.last + 1 : 0u, c.open ? 1u : 0u};
        if (d->burst_scratch.reserve((size_t)2 * kBurstTileWords * a.n_tiles) != hipSuccess || d->burst_total.reserve(8) != hipSuccess) {
            (void)hipGetLastError();
            return d->fail("%s: cannot allocate the %u tiles' %zu bytes on the device", what, a.n_tiles,
                           (size_t)2 * kBurstTileWords * a.n_tiles * sizeof(uint32_t));
        }
        a.summaries = d->burst_scratch;
        a.rows = d->burst_scratch + (size_t)kBurstTileWords * a.n_tiles;
        a.total = d->burst_total.dev;
        HIP_TRY(d, launch_burst_slice_count(a, sl, d->stream));
        HIP_TRY(d, hipMemcpyAsync(d->burst_total.host, d->burst_total.dev, sizeof(uint32_t), hipMemcpyDeviceToHost, d->stream));
        WAIT_STREAM(d, d->stream, "the scan stream");
        total = d->burst_total.host[0];
        if (total) {
            n_out = std::min<size_t>(total - 1, cap);
            if (d->burst_tab.reserve(4 * (n_out + 1)) != hipSuccess) {
                (void)hipGetLastError();
                return d->fail("%s: cannot allocate a table of %zu bursts on the device", what, n_out + 1);
            }
            a.table = d->burst_tab;
            a.cap = (uint32_t)n_out;
            adsb_burst *back = reinterpret_cast<adsb_burst *>(d->burst_total.host.p + 4);
            HIP_TRY(d, hipMemsetAsync(d->burst_tab, 0, (n_out + 1) * sizeof(adsb_burst), d->stream));
            HIP_TRY(d, launch_burst_slice_emit(a, sl, d->stream));
            if (n_out)
                HIP_TRY(d, hipMemcpyAsync(bursts, d->burst_tab, n_out * sizeof(adsb_burst), hipMemcpyDeviceToHost, d->stream));
            HIP_TRY(d, hipMemcpyAsync(back, d->burst_tab + 4 * n_out, sizeof(adsb_burst), hipMemcpyDeviceToHost, d->stream));
            WAIT_STREAM(d, d->stream, "the scan stream");
            last = *back;
        }
    }
    adsb_burst_carry next{};
    next.runs = seen;
    if (total == 0) {
        *out = next;
        return 0;
    }
    if (c.open) { // what the carried cluster had before this slice: into burst 0, which the kernels gave only what the slice adds
        adsb_burst *first = total == 1 ? &last : n_out ? &bursts[0] : nullptr;
        if (first) {
            first->begin = total == 1 ? c.first : c.first >= lead ? c.first - lead : 0u;
            if (first->end == 0) // (no hot run of the slice joined it)
                first->end = total == 1 ? c.last + 1 : c.last + hang + 1;
            first->hot += c.hot;
            first->peak = larger_bits(first->peak, c.peak);
        }
    }
    const uint64_t e = last.end - 1;
    if (!final && e + join >= seen) { // a run that is still to come may join it
        next.open = 1, next.first = last.begin, next.last = (uint32_t)e, next.hot = last.hot, next.peak = last.peak;
        *out = next;
        return (long)total - 1;
    }
    if (total - 1 < cap)
        bursts[total - 1] = adsb_burst{last.begin >= lead ? last.begin - lead : 0u, (uint32_t)std::min<uint64_t>(seen, e + hang + 1), last.hot, last.peak};
    *out = next;
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

long adsb_bursts_slice_device(adsb_decoder *d, const float *device_env, size_t n_env, float threshold, uint32_t lead, uint32_t hang,
                              const adsb_burst_carry *in, int final, adsb_burst *bursts, size_t cap, adsb_burst_carry *out)
{
    const char *what = "adsb_bursts_slice_device";
    if (!d)
        return -1;
    if (bursts_refusal(d, what, "device", device_env, n_env, threshold, lead, hang, bursts, cap) || bursts_slice_refusal(d, what, n_env, in, out))
        return -1;
    return bursts_slice_run(d, what, device_env, n_env, threshold, lead, hang, *in, final, bursts, cap, out);
}

long adsb_bursts_slice_host(adsb_decoder *d, const float *env, size_t n_env, float threshold, uint32_t lead, uint32_t hang,
                            const adsb_burst_carry *in, int final, adsb_burst *bursts, size_t cap, adsb_burst_carry *out)
{
    const char *what = "adsb_bursts_slice_host";
    if (!d)
        return -1;
    if (bursts_refusal(d, what, "host", env, n_env, threshold, lead, hang, bursts, cap) || bursts_slice_refusal(d, what, n_env, in, out))
        return -1;
    if (n_env) {
        HIP_TRY(d, hipSetDevice(d->device));
        if (d->pow_buf.reserve((n_env + 65535) & ~(size_t)65535) != hipSuccess) {
            (void)hipGetLastError();
            return d->fail("%s: cannot allocate the envelope's %zu bytes on the device", what, n_env * sizeof(float));
        }
        HIP_TRY(d, hipMemcpyAsync(d->pow_buf, env, n_env * sizeof(float), hipMemcpyHostToDevice, d->copy_stream[0]));
        WAIT_STREAM(d, d->copy_stream[0], "a copy stream");
    }
    return bursts_slice_run(d, what, d->pow_buf, n_env, threshold, lead, hang, *in, final, bursts, cap, out);
}

} // extern "C"
