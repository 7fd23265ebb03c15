// decoder_level_windows.hip -- the level reports of K consecutive windows of ONE stream (include/adsbdec_amd.h: adsb_level_windows,
// adsb_level_windows_host): window i's report is that of the power samples [edges[i], edges[i + 1]) of the stream -- the floats
// adsb_power_window writes for them, the six older pairs of every sample taken from the buffer where it holds them -- with the rail
// counters of the codes of their own pairs, and one envelope serves all windows (the definition is adsbdec_amd/levels.py
// level_windows).  Up to kLevelBatchCaptures windows cost ONE level launch (level_windows_kernel.hip), one memset of their totals and
// one copy of them back, through the table and the totals the batch level calls use (decoder_level_batch.hip); more windows go in
// such sub-launches.  Stateless as the export's window call is: neither the handle's stream position nor its resolver changes; the
// launches go to the scan stream, behind whatever a push has left there, and the call returns when the reports are in out[].
// Every refusal comes before anything is launched, written or counted.  (The handle: decoder_state.hpp.)
#include "decoder_state.hpp"
#include "level.h"
#include "level_windows.hpp"

using namespace adsb;

namespace {

// The refusals of adsb_level_windows*, in one pass: the window call's of the buffer (adsb_power_window's rules 1 to 3), the edges
// window by window, the single level call's of report and envelope.  in_align: bytes a device input pointer is aligned to (0: host
// memory, any).
int level_windows_refusal(adsb_decoder *d, const char *what, const void *samples, unsigned in_align, uint64_t first_sample, size_t n,
                          size_t n_windows, const uint64_t *edges, const adsb_level_report *out, const float *env, size_t env_cap)
{
    if ((uint64_t)n_windows > kExportMaxCaptures)
        return d->fail("%s: %zu windows: the table of a launch indexes its rows in 32 bits", what, n_windows);
    if (!edges || !out)
        return d->fail("%s: NULL %s", what, !edges ? "edges" : "reports");
    if (shard_too_long(d, what, first_sample, n, 0)) // (on a long-stream handle too, as adsb_power_window)
        return -1;
    if (first_sample % 8)
        return d->fail("%s: buffer must start at a multiple of 8 samples", what);
    if (in_align && (uintptr_t)samples % in_align)
        return d->fail("%s: buffer must start %u-byte aligned (%p)", what, in_align, samples);
    for (size_t i = 0; i < n_windows; i++) {
        if (edges[i] % kRun)
            return d->fail("%s: window %zu starts at power sample %llu: every edge but the last must be a multiple of 28", what, i,
                           (unsigned long long)edges[i]);
        if (edges[i + 1] < edges[i])
            return d->fail("%s: window %zu ends at %llu, below its start %llu: the edges must ascend", what, i,
                           (unsigned long long)edges[i + 1], (unsigned long long)edges[i]);
    }
    const uint64_t m_begin = edges[0], m_end = edges[n_windows]; // (ascending: the smallest and the largest)
    if (m_end > (1ull << 31) || 2 * m_begin < first_sample || 2 * m_end > first_sample + n)
        return d->fail("%s: the buffer does not hold the own pair of every power sample of %s (2 edges[0] >= first_sample and "
                       "2 edges[%zu] <= first_sample + n)", what, 2 * m_begin < first_sample ? "window 0" : "the last window", n_windows);
    if (m_end > m_begin && !samples)
        return d->fail("%s: NULL buffer", what);
    if (!env && env_cap)
        return d->fail("%s: NULL envelope with env_cap = %zu (no envelope: NULL and 0)", what, env_cap);
    if (env && (uintptr_t)env % 4)
        return d->fail("%s: the envelope must be 4-byte aligned (%p)", what, (const void *)env);
    if (env && env_cap < env_floats(m_end - m_begin))
        return d->fail("%s: the envelope of %llu power samples has %zu floats, the array holds %zu", what, (unsigned long long)(m_end - m_begin),
                       env_floats(m_end - m_begin), env_cap);
    return 0;
}

// The checked windows over the uint16 samples at device_u16 (sample first_sample of the stream on, n of them), in sub-launches of
// kLevelBatchCaptures windows on the scan stream, each waited for: the table and the totals are the next one's to rewrite.  The
// reports go to rep[] (host memory of the caller's or of this unit's), the envelope to device_env.
long level_windows(adsb_decoder *d, const char *what, const void *device_u16, uint64_t first_sample, size_t n, size_t n_windows,
                   const uint64_t *edges, adsb_level_report *rep, float *device_env)
{
    static_assert(sizeof(adsb_level_report) == kLevelWords * sizeof(unsigned long long), "level.h kLevelWords");
    const int64_t pbuf0 = (int64_t)(first_sample / 2), p_hi = (int64_t)((first_sample + n) / 2);
    std::vector<uint32_t> row_of;
    for (size_t c0 = 0; c0 < n_windows; c0 += kLevelBatchCaptures) {
        const size_t k = std::min(kLevelBatchCaptures, n_windows - c0);
        const uint64_t *e = edges + c0;
        row_of.assign(k, UINT32_MAX);
        size_t rows_max = 0;
        for (size_t i = 0; i < k; i++)
            rows_max += e[i + 1] > e[i];
        if (rows_max) {
            // (every earlier launch that read the table or added to the totals has been waited for)
            if (d->level_tab.reserve((rows_max + 1) * sizeof(WindowSeg)) != hipSuccess || d->level_batch.reserve(rows_max * kLevelWords) != hipSuccess) {
                (void)hipGetLastError();
                return d->fail("%s: cannot allocate the %zu bytes of the reports of %zu windows on the device and pinned", what,
                               rows_max * kLevelWords * sizeof(unsigned long long), rows_max);
            }
            WindowSeg *tab = reinterpret_cast<WindowSeg *>(d->level_tab.host.p);
            uint64_t units = 0;
            const uint32_t rows = level_windows_table(k, e, tab, row_of.data(), &units);
            const size_t bytes = (size_t)rows * kLevelWords * sizeof(unsigned long long);
            HIP_TRY(d, hipMemcpyAsync(d->level_tab.dev, d->level_tab.host, ((size_t)rows + 1) * sizeof(WindowSeg), hipMemcpyHostToDevice, d->stream));
            HIP_TRY(d, hipMemsetAsync(d->level_batch.dev, 0, bytes, d->stream));
            HIP_TRY(d, launch_level_windows(static_cast<const uint32_t *>(device_u16), pbuf0, p_hi, (int64_t)edges[0],
                                            reinterpret_cast<const WindowSeg *>(d->level_tab.dev.p), rows, units, d->level_batch.dev, device_env,
                                            (unsigned)std::max(0, d->level_batch_blocks), d->stream));
            HIP_TRY(d, hipMemcpyAsync(d->level_batch.host, d->level_batch.dev, bytes, hipMemcpyDeviceToHost, d->stream));
            WAIT_STREAM(d, d->stream, "the scan stream");
        }
        for (size_t i = 0; i < k; i++) {
            if (row_of[i] == UINT32_MAX) {
                memset(&rep[c0 + i], 0, sizeof rep[0]);
                continue;
            }
            memcpy(&rep[c0 + i], d->level_batch.host.p + (size_t)row_of[i] * kLevelWords, sizeof rep[0]);
            rep[c0 + i].samples = e[i + 1] - e[i];
        }
    }
    return (long)(edges[n_windows] - edges[0]);
}

} // namespace

extern "C" {

long adsb_level_windows(adsb_decoder *d, const void *device_samples, uint64_t first_sample, size_t n, size_t n_windows, const uint64_t *edges,
                        adsb_level_report *out, float *device_env, size_t env_cap)
{
    const char *what = "adsb_level_windows";
    if (!d)
        return -1;
    if (level_windows_refusal(d, what, device_samples, 16, first_sample, n, n_windows, edges, out, device_env, env_cap))
        return -1;
    if (n_windows == 0)
        return 0;
    HIP_TRY(d, hipSetDevice(d->device));
    return level_windows(d, what, device_samples, first_sample, n, n_windows, edges, out, device_env);
}

long adsb_level_windows_host(adsb_decoder *d, const uint16_t *samples, uint64_t first_sample, size_t n, size_t n_windows, const uint64_t *edges,
                             adsb_level_report *out, float *env, size_t env_cap)
{
    const char *what = "adsb_level_windows_host";
    if (!d)
        return -1;
    if (level_windows_refusal(d, what, samples, 0, first_sample, n, n_windows, edges, out, env, env_cap))
        return -1;
    if (n_windows == 0)
        return 0;
    const uint64_t m = edges[n_windows] - edges[0];
    if (m == 0) {
        memset(out, 0, n_windows * sizeof out[0]);
        return 0;
    }
    const size_t ef = env ? env_floats(m) : 0;
    if (window_in(d, samples, n, ef) || level_windows(d, what, d->win_buf, first_sample, n, n_windows, edges, out, ef ? d->pow_buf.p : nullptr) < 0 ||
        (ef && floats_out(d, env, ef)))
        return -1;
    return (long)m;
}

} // extern "C"
