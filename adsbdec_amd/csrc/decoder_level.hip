// decoder_level.hip -- the level calls (include/adsbdec_amd.h: adsb_level_*): a capture's power samples -- exactly the floats the
// export call of the same flavour writes (decoder_export.hip) -- reduced on the GPU to an adsb_level_report and, where asked for, an
// envelope of one float per 28 power samples (level_kernel.hip; the definition is adsbdec_amd/levels.py level_report).  Stateless as
// the export calls are: a call changes neither the handle's stream position nor its resolver; its kernels go to the scan stream,
// behind whatever a push has left there, and the call returns when the report is in *out.  A refusal writes nothing.
#include "decoder_state.hpp"
#include "level.h"

using namespace adsb;

namespace {

// What every level call asks of its report and its envelope, behind the flavour's own checks of the samples.
int level_out_refusal(adsb_decoder *d, const char *what, uint64_t m, const adsb_level_report *out, const float *env, size_t env_cap)
{
    if (!out)
        return d->fail("%s: NULL report", what);
    if (!env && env_cap)
        return d->fail("%s: NULL envelope with env_cap = %zu (no envelope: NULL and 0)", what, env_cap);
    if (env && (uintptr_t)env % 4)
        return d->fail("%s: the envelope must be 4-byte aligned (%p)", what, (const void *)env);
    if (env && (env_cap == 0 || env_cap < env_floats(m)))
        return d->fail("%s: the envelope of %llu power samples has %zu floats, the array holds %zu", what, (unsigned long long)m,
                       env_floats(m), env_cap);
    return 0;
}

// the real flavours' checks of a capture of n uint16 codes (those of adsb_power_device: export rules 1 and 3)
int level_real_refusal(adsb_decoder *d, const char *what, size_t n)
{
    return shard_too_long(d, what, 0, n, 0) ? -1 : 0;
}

// the totals, zeroed on the scan stream
int level_begin(adsb_decoder *d, const char *what)
{
    HIP_TRY(d, hipSetDevice(d->device));
    if (d->level.reserve(kLevelWords + 1) != hipSuccess || // (+ 1: a real capture's last codes, level_end)
        (level_uses_rows() && d->level_rows.reserve((size_t)kLevelRowWords * level_max_blocks()) != hipSuccess)) {
        (void)hipGetLastError();
        return d->fail("%s: cannot allocate the report's %zu bytes on the device", what, kLevelWords * sizeof(unsigned long long));
    }
    HIP_TRY(d, hipMemsetAsync(d->level.dev, 0, kLevelWords * sizeof(unsigned long long), d->stream));
    return 0;
}

// behind the launch: the totals back, and the wait.  tail_n (0 .. 3): the codes of a real capture behind its last whole group of
// four, at tail_dev -- they make no power sample (air.c:59) but they are samples of the capture, and the rail counters are the
// capture's: they come back beside the totals and are counted here.
long level_end(adsb_decoder *d, uint64_t m, adsb_level_report *out, const uint16_t *tail_dev = nullptr, unsigned tail_n = 0)
{
    HIP_TRY(d, hipMemcpyAsync(d->level.host, d->level.dev, kLevelWords * sizeof(unsigned long long), hipMemcpyDeviceToHost, d->stream));
    uint16_t *tail = reinterpret_cast<uint16_t *>(d->level.host.p + kLevelWords);
    if (tail_n)
        HIP_TRY(d, hipMemcpyAsync(tail, tail_dev, tail_n * sizeof(uint16_t), hipMemcpyDeviceToHost, d->stream));
    WAIT_STREAM(d, d->stream, "the scan stream");
    static_assert(sizeof(adsb_level_report) == kLevelWords * sizeof(unsigned long long), "level.h kLevelWords");
    memcpy(out, d->level.host.p, sizeof *out);
    out->samples = m;
    for (unsigned i = 0; i < tail_n; i++) {
        out->rail_lo += tail[i] == 0;
        out->rail_hi += tail[i] == 4095;
        out->over += tail[i] > 4095;
    }
    return (long)m;
}

long level_empty(adsb_level_report *out)
{
    memset(out, 0, sizeof *out);
    return 0;
}

// a whole capture of n uint16 codes in HBM as a fresh stream (checked by the caller); on the scan stream, behind what made it
long level_capture(adsb_decoder *d, const char *what, const void *device_u16, size_t n, adsb_level_report *out, float *env)
{
    const uint64_t m = power_samples_produced(n);
    if (level_begin(d, what))
        return -1;
    HIP_TRY(d, launch_level(static_cast<const uint32_t *>(device_u16), (int64_t)(n / 2), (int64_t)m, d->level.dev, env, d->level_rows, d->stream));
    return level_end(d, m, out, static_cast<const uint16_t *>(device_u16) + 4 * (n / 4), (unsigned)(n % 4));
}

// A capture of the flavour F in device memory: the flavour's checks of the samples where the entry point has not made them (the real
// flavours': a uint16 capture is read where it lies and says so in the export's words), the report's and the envelope's, what the
// flavour puts in front (decoder_stage.hip), and the launch behind it on the same stream.
long level_device(adsb_decoder *d, const char *what, const Flavour &F, const void *device_samples, size_t n, adsb_level_report *out,
                  float *device_env, size_t env_cap)
{
    const uint64_t m = F.power_samples(n);
    if (F.real()) {
        if (F.groups8 && n % kPackedGroupSamples)
            return d->fail("%s: n = %zu is not a multiple of 8 (packed samples come in groups of 8 in 12 bytes)", what, n);
        if ((uintptr_t)device_samples % F.in_align)
            return F.front == Flavour::kNone ? d->fail("%s: buffer must start 16-byte aligned (%p)", what, device_samples)
                                             : d->fail("%s: device pointer %p is not %zu-byte aligned", what, device_samples, (size_t)F.in_align);
        if (level_real_refusal(d, what, n))
            return -1;
    }
    if (level_out_refusal(d, what, m, out, device_env, env_cap))
        return -1;
    if (m == 0)
        return level_empty(out);
    if (!device_samples)
        return d->fail("%s: NULL buffer", what);
    const void *p = flavour_to_scratch(d, what, F, device_samples, n);
    if (!p)
        return -1;
    if (F.real())
        return level_capture(d, what, p, n, out, device_env);
    if (level_begin(d, what)) // n units at p that ARE power samples
        return -1;
    HIP_TRY(d, launch_level_units(F.level_kind, p, n, d->level.dev, device_env, d->level_rows, d->stream));
    return level_end(d, n, out);
}

} // namespace

extern "C" {

long adsb_level_device(adsb_decoder *d, const void *device_samples, size_t n, adsb_level_report *out, float *device_env, size_t env_cap)
{
    return d ? level_device(d, "adsb_level_device", flavour_uint16(), device_samples, n, out, device_env, env_cap) : -1;
}

long adsb_level_device_as(adsb_decoder *d, int fmt, const void *device_samples, size_t n, adsb_level_report *out, float *device_env,
                          size_t env_cap)
{
    const char *what = "adsb_level_device_as";
    Flavour F;
    if (!d)
        return -1;
    const int k = flavour_as(d, what, fmt, &F);
    if (k < 0)
        return -1;
    if (k)
        return adsb_level_device(d, device_samples, n, out, device_env, env_cap);
    return level_device(d, what, F, device_samples, n, out, device_env, env_cap);
}

long adsb_level_device_packed(adsb_decoder *d, const void *device_packed, size_t n, adsb_level_report *out, float *device_env, size_t env_cap)
{
    return d ? level_device(d, "adsb_level_device_packed", flavour_packed(), device_packed, n, out, device_env, env_cap) : -1;
}

long adsb_level_device_iq(adsb_decoder *d, int fmt, const void *device_samples, size_t n, adsb_level_report *out, float *device_env,
                          size_t env_cap)
{
    const char *what = "adsb_level_device_iq";
    if (!d || iq_refusal(d, what, fmt, device_samples, n, true, 0))
        return -1;
    return level_device(d, what, flavour_of_iq(fmt), device_samples, n, out, device_env, env_cap);
}

long adsb_level_device_power(adsb_decoder *d, const void *device_samples, size_t n, adsb_level_report *out, float *device_env, size_t env_cap)
{
    const char *what = "adsb_level_device_power";
    if (!d || power_refusal(d, what, device_samples, n, true, 0))
        return -1;
    return level_device(d, what, flavour_power(), device_samples, n, out, device_env, env_cap);
}

long adsb_level_host(adsb_decoder *d, const uint16_t *samples, size_t n, adsb_level_report *out, float *env, size_t env_cap)
{
    const char *what = "adsb_level_host";
    if (!d)
        return -1;
    const uint64_t m = power_samples_produced(n);
    if (level_real_refusal(d, what, n) || level_out_refusal(d, what, m, out, env, env_cap))
        return -1;
    if (m == 0)
        return level_empty(out);
    if (!samples)
        return d->fail("%s: NULL buffer", what);
    const size_t ef = env ? env_floats(m) : 0;
    adsb_level_report r;
    if (window_in(d, samples, n, ef) || level_capture(d, what, d->win_buf, n, &r, ef ? d->pow_buf.p : nullptr) < 0 || (ef && floats_out(d, env, ef)))
        return -1;
    *out = r;
    return (long)m;
}

} // extern "C"
