// decoder_level_batch.hip -- the level calls of a BATCH of captures (include/adsbdec_amd.h: adsb_level_batch_*): capture i's report,
// and where asked its envelope, are what the single call of the same flavour (decoder_level.hip) gives for it alone, and a
// sub-batch of up to kLevelBatchCaptures captures costs ONE level launch (level_batch_kernel.hip) behind at most one unpack or
// conversion launch (decoder_batch.hip's, into the scratch the batch decodes use), one memset of its totals and one copy of them
// back -- no copy per capture, a real capture's trailing n % 4 codes included (the launch counts them).  Stateless as the single
// calls are: neither the handle's stream position nor its resolver changes; the launches go to the scan stream, behind whatever a
// push has left there, and the call returns when the reports are in out[].  Every refusal comes before anything is launched,
// written or counted.  (The handle: decoder_state.hpp.)
#include "decoder_state.hpp"
#include "level.h"
#include "level_batch.hpp"

using namespace adsb;

namespace {

// The refusals of adsb_level_batch_*, by capture, before anything is launched: the batch export's (decoder_export_batch.hip
// export_batch_refusal) of the samples, the single level call's (decoder_level.hip level_out_refusal) of report and envelope.
int level_batch_refusal(adsb_decoder *d, const char *what, const Flavour &F, size_t n_captures, const void *const *src,
                        const size_t *n, const adsb_level_report *out, float *const *env, const size_t *env_cap)
{
    if ((uint64_t)n_captures > kExportMaxCaptures)
        return d->fail("%s: %zu captures: the table of a batch indexes its rows in 32 bits", what, n_captures);
    if (!out)
        return d->fail("%s: NULL reports", what);
    if (n_captures && (!src || !n))
        return d->fail("%s: NULL capture arrays", what);
    if (!env != !env_cap)
        return d->fail("%s: the envelope arrays are both NULL (no envelope for any capture) or both given", what);
    for (size_t i = 0; i < n_captures; i++) {
        if (!F.real() && (uint64_t)n[i] >= (1ull << 31))
            return d->fail("%s: capture %zu has %zu %s samples: 2^31 or more; such streams end below", what, i, n[i],
                           F.kind == kKindPower ? "power" : "complex");
        if (batch_samples_refusal(d, what, i, src[i], n[i], F))
            return -1;
        const uint64_t m = F.power_samples(n[i]);
        if (env) {
            if (!env[i] && env_cap[i])
                return d->fail("%s: capture %zu: NULL envelope with env_cap = %zu (no envelope: NULL and 0)", what, i, env_cap[i]);
            if (env[i] && (uintptr_t)env[i] % 4)
                return d->fail("%s: capture %zu: the envelope must be 4-byte aligned (%p)", what, i, (const void *)env[i]);
            if (env[i] && (env_cap[i] == 0 || env_cap[i] < env_floats(m)))
                return d->fail("%s: capture %zu: the envelope of %llu power samples has %zu floats, the array holds %zu", what, i,
                               (unsigned long long)m, env_floats(m), env_cap[i]);
        }
        if (m && !src[i])
            return d->fail("%s: capture %zu: NULL buffer", what, i);
    }
    return 0;
}

// One sub-batch of k checked captures on `st`: capture i's samples (uint16 real ones, or the units of F.kind) are in device memory
// at at[i], its envelope (env != NULL and env[i] != NULL) goes to env[i] in device memory.  The table, the zeroed totals, the launch,
// the totals back into the pinned half; not waited for.  row_of[i]: which of the totals are capture i's (level_batch.hpp).
// tail_on_device: the launch counts a real capture's trailing n % 4 codes.
int level_sub_launch(adsb_decoder *d, const char *what, const Flavour &F, size_t k, const void *const *at, const size_t *n,
                     float *const *env, bool tail_on_device, hipStream_t st, std::vector<uint32_t> &row_of)
{
    std::vector<uint64_t> m(k), p_hi(k), tail(k);
    row_of.assign(k, UINT32_MAX);
    size_t rows_max = 0;
    for (size_t i = 0; i < k; i++) {
        m[i] = F.power_samples(n[i]);
        p_hi[i] = n[i] / 2;
        tail[i] = tail_on_device ? n[i] % 4 : 0;
        rows_max += m[i] != 0;
    }
    if (rows_max == 0)
        return 0;
    // (every earlier launch that read the table or added to the totals has been waited for)
    if (d->level_tab.reserve((rows_max + 1) * sizeof(LevelSeg)) != hipSuccess || d->level_batch.reserve(rows_max * kLevelWords) != hipSuccess) {
        (void)hipGetLastError();
        return d->fail("%s: cannot allocate the %zu bytes of the reports of %zu captures on the device and pinned", what,
                       rows_max * kLevelWords * sizeof(unsigned long long), rows_max);
    }
    LevelSeg *tab = reinterpret_cast<LevelSeg *>(d->level_tab.host.p);
    uint64_t units = 0;
    const bool real = F.real();
    const uint32_t rows = level_table(k, m.data(), real ? p_hi.data() : nullptr, real ? tail.data() : nullptr, at, env, tab, row_of.data(), &units);
    const size_t bytes = (size_t)rows * kLevelWords * sizeof(unsigned long long);
    HIP_TRY(d, hipMemcpyAsync(d->level_tab.dev, d->level_tab.host, ((size_t)rows + 1) * sizeof(LevelSeg), hipMemcpyHostToDevice, st));
    HIP_TRY(d, hipMemsetAsync(d->level_batch.dev, 0, bytes, st));
    HIP_TRY(d, launch_level_batch(F.level_kind, reinterpret_cast<const LevelSeg *>(d->level_tab.dev.p), rows, units, d->level_batch.dev,
                                  (unsigned)std::max(0, d->level_batch_blocks), st));
    HIP_TRY(d, hipMemcpyAsync(d->level_batch.host, d->level_batch.dev, bytes, hipMemcpyDeviceToHost, st));
    return 0;
}

// ... behind the wait: the reports of the sub-batch's captures
void level_sub_reports(const adsb_decoder *d, const Flavour &F, size_t k, const size_t *n, const std::vector<uint32_t> &row_of,
                       adsb_level_report *out)
{
    static_assert(sizeof(adsb_level_report) == kLevelWords * sizeof(unsigned long long), "level.h kLevelWords");
    for (size_t i = 0; i < k; i++) {
        if (row_of[i] == UINT32_MAX) {
            memset(&out[i], 0, sizeof out[i]);
            continue;
        }
        memcpy(&out[i], d->level_batch.host.p + (size_t)row_of[i] * kLevelWords, sizeof out[i]);
        out[i].samples = F.power_samples(n[i]);
    }
}

// A checked batch in sub-batches of kLevelBatchCaptures, each behind what the flavour puts in front (decoder_stage.hip), on the scan
// stream and waited for: the scratch, the table and the totals are the next sub-batch's to rewrite.  Returns the power samples
// reported in all, or -1.
long level_batch(adsb_decoder *d, const char *what, const Flavour &F, size_t n_captures, const void *const *src, const size_t *n,
                 adsb_level_report *out, float *const *env, const size_t *env_cap)
{
    if (level_batch_refusal(d, what, F, n_captures, src, n, out, env, env_cap))
        return -1;
    HIP_TRY(d, hipSetDevice(d->device));
    uint64_t total = 0;
    std::vector<uint32_t> row_of;
    std::vector<const void *> at;
    for (size_t c0 = 0; c0 < n_captures; c0 += kLevelBatchCaptures) {
        const size_t k = std::min(kLevelBatchCaptures, n_captures - c0);
        if (flavour_batch_to_scratch(d, what, F, k, src + c0, n + c0, at) ||
            level_sub_launch(d, what, F, k, at.data(), n + c0, env ? env + c0 : nullptr, true, d->stream, row_of))
            return -1;
        WAIT_STREAM(d, d->stream, "the scan stream");
        level_sub_reports(d, F, k, n + c0, row_of, out + c0);
        for (size_t i = 0; i < k; i++)
            total += F.power_samples(n[c0 + i]);
    }
    return (long)total;
}

} // namespace

extern "C" {

long adsb_level_batch_device(adsb_decoder *d, size_t n_captures, const void *const *device_samples, const size_t *n, adsb_level_report *out,
                             float *const *device_env, const size_t *env_cap)
{
    return d ? level_batch(d, "adsb_level_batch_device", flavour_uint16(), n_captures, device_samples, n, out, device_env, env_cap) : -1;
}

long adsb_level_batch_device_as(adsb_decoder *d, int fmt, size_t n_captures, const void *const *device_samples, const size_t *n,
                                adsb_level_report *out, float *const *device_env, const size_t *env_cap)
{
    const char *what = "adsb_level_batch_device_as";
    Flavour F;
    if (!d)
        return -1;
    const int k = flavour_as(d, what, fmt, &F);
    if (k < 0)
        return -1;
    if (k)
        return adsb_level_batch_device(d, n_captures, device_samples, n, out, device_env, env_cap);
    return level_batch(d, what, F, n_captures, device_samples, n, out, device_env, env_cap);
}

long adsb_level_batch_device_packed(adsb_decoder *d, size_t n_captures, const void *const *device_packed, const size_t *n,
                                    adsb_level_report *out, float *const *device_env, const size_t *env_cap)
{
    return d ? level_batch(d, "adsb_level_batch_device_packed", flavour_packed(), n_captures, device_packed, n, out, device_env, env_cap) : -1;
}

long adsb_level_batch_device_iq(adsb_decoder *d, int fmt, size_t n_captures, const void *const *device_samples, const size_t *n,
                                adsb_level_report *out, float *const *device_env, const size_t *env_cap)
{
    const char *what = "adsb_level_batch_device_iq";
    Flavour F;
    if (!d || flavour_iq(d, what, fmt, &F))
        return -1;
    return level_batch(d, what, F, n_captures, device_samples, n, out, device_env, env_cap);
}

long adsb_level_batch_device_power(adsb_decoder *d, size_t n_captures, const void *const *device_samples, const size_t *n,
                                   adsb_level_report *out, float *const *device_env, const size_t *env_cap)
{
    return d ? level_batch(d, "adsb_level_batch_device_power", flavour_power(), n_captures, device_samples, n, out, device_env, env_cap) : -1;
}

long adsb_level_batch_host(adsb_decoder *d, size_t n_captures, const uint16_t *const *samples, const size_t *n, adsb_level_report *out,
                           float *const *env, const size_t *env_cap)
{
    const char *what = "adsb_level_batch_host";
    if (!d)
        return -1;
    const Flavour F = flavour_uint16().on_host(), kDevice = flavour_uint16();
    const void *const *src = reinterpret_cast<const void *const *>(samples);
    if (level_batch_refusal(d, what, F, n_captures, src, n, out, env, env_cap))
        return -1;
    HIP_TRY(d, hipSetDevice(d->device));
    // per sub-batch: every capture at a 128-byte boundary of the scratch adsb_decode_batch_host lands its captures in, every
    // envelope at a 128-byte boundary of adsb_power_window_host's array; copies in, launch and copies out on ONE copy stream, in
    // order.  The trailing n % 4 codes are counted here, from the caller's memory.
    hipStream_t cs = d->copy_stream[0];
    uint64_t total = 0;
    std::vector<uint32_t> row_of;
    for (size_t c0 = 0; c0 < n_captures; c0 += kLevelBatchCaptures) {
        const size_t k = std::min(kLevelBatchCaptures, n_captures - c0);
        // (a capture without a power sample takes no room in either)
        std::vector<size_t> in_bytes(k), floats(k);
        size_t in_all = 0, env_all = 0;
        for (size_t i = 0; i < k; i++) {
            const uint64_t m = power_samples_produced(n[c0 + i]);
            in_bytes[i] = m ? n[c0 + i] * sizeof(uint16_t) : 0;
            floats[i] = m && env && env[c0 + i] ? env_floats(m) : 0;
            in_all += in_bytes[i];
            env_all += floats[i];
        }
        if (in_all == 0) {
            for (size_t i = 0; i < k; i++)
                memset(&out[c0 + i], 0, sizeof out[0]);
            continue;
        }
        std::vector<const void *> at;
        std::vector<float *> env_dev(k, nullptr);
        if ((env_all && pow_slots(d, k, floats.data(), env_dev)) ||
            land_captures(d, what, d->batch_in, "the captures", k, src + c0, in_bytes.data(), 128, Land::FirstCopyStream, at))
            return -1;
        if (level_sub_launch(d, what, kDevice, k, at.data(), n + c0, env_all ? env_dev.data() : nullptr, false, cs, row_of) ||
            (env_all && pow_slots_out(d, k, env + c0, env_dev, floats.data(), cs)))
            return -1;
        WAIT_STREAM(d, cs, "a copy stream");
        level_sub_reports(d, kDevice, k, n + c0, row_of, out + c0);
        for (size_t i = 0; i < k; i++) {
            const uint64_t m = power_samples_produced(n[c0 + i]);
            total += m;
            if (m == 0)
                continue;
            for (size_t j = 4 * (n[c0 + i] / 4); j < n[c0 + i]; j++) {
                const uint16_t code = samples[c0 + i][j];
                out[c0 + i].rail_lo += code == 0;
                out[c0 + i].rail_hi += code == 4095;
                out[c0 + i].over += code > 4095;
            }
        }
    }
    return (long)total;
}

int adsb_debug_set_level_batch_blocks(adsb_decoder *d, int blocks)
{
    if (!d)
        return -1;
    if (blocks < 0)
        return d->fail("adsb_debug_set_level_batch_blocks: %d workgroups (0: the default; else the most a batch level launch may have)", blocks);
    d->level_batch_blocks = blocks;
    return 0;
}

} // extern "C"
