// decoder_export_batch.hip -- the export calls of a BATCH of captures (include/adsbdec_amd.h: adsb_power_batch_*): capture i's power
// samples are what the single call of the same flavour (decoder_export.hip) writes for it alone, bit for bit, and the whole batch
// costs ONE export launch (power_export_batch_kernel.hip) behind at most one unpack or conversion launch (decoder_batch.hip's, into
// the scratch the batch decodes use).  Stateless as the single calls are: neither the handle's stream position nor its resolver
// changes; the launches go to the scan stream, behind whatever a push has left there, and the call returns when the floats are
// written.  Every refusal comes before anything is launched or counted.  (The handle: decoder_state.hpp.)
#include "decoder_state.hpp"
#include "power_export_batch.hpp"

using namespace adsb;

namespace {

// The refusals of adsb_power_batch_*, by capture, before anything is launched.  out_device: the output pointers are device memory,
// 16-byte aligned.
int export_batch_refusal(adsb_decoder *d, const char *what, const Flavour &F, bool out_device, size_t n_captures, const void *const *src,
                         const size_t *n, float *const *out, const size_t *cap)
{
    if ((uint64_t)n_captures > kExportMaxCaptures)
        return d->fail("%s: %zu captures: the table of a batch indexes its rows in 32 bits", what, n_captures);
    if (n_captures && (!src || !n || !out || !cap))
        return d->fail("%s: NULL capture arrays", what);
    for (size_t i = 0; i < n_captures; i++) {
        if (!F.real() && (uint64_t)n[i] >= (1ull << 31))
            return d->fail("%s: capture %zu has %zu complex samples: 2^31 or more; IQ streams end below", what, i, n[i]);
        if (batch_samples_refusal(d, what, i, src[i], n[i], F))
            return -1;
        if (out_device && (uintptr_t)out[i] % 16 != 0)
            return d->fail("%s: capture %zu: the power array must be 16-byte aligned (%p)", what, i, (const void *)out[i]);
        const uint64_t count = F.power_samples(n[i]);
        if (count > cap[i])
            return d->fail("%s: capture %zu has %llu power samples, the array holds %zu", what, i, (unsigned long long)count, cap[i]);
        if (count && (!src[i] || !out[i]))
            return d->fail("%s: capture %zu: NULL buffer", what, i);
    }
    return 0;
}

// The export launch of a checked batch on `st`, behind its table's upload: capture i's samples (uint16 real ones, or int16 complex
// ones) are in device memory at at[i].  Not waited for.  Returns the floats the launch writes, or -1.
long export_batch_launch(adsb_decoder *d, const Flavour &F, size_t n_captures, const void *const *at, const size_t *n,
                         float *const *out, hipStream_t st)
{
    std::vector<uint64_t> m(n_captures), p_hi(n_captures);
    uint64_t total = 0;
    for (size_t i = 0; i < n_captures; i++) {
        m[i] = F.power_samples(n[i]);
        p_hi[i] = n[i] / 2;
        total += m[i];
    }
    if (total == 0)
        return 0;
    HIP_TRY(d, d->export_tab.reserve((n_captures + 1) * sizeof(ExportSeg))); // (every earlier launch that read it has been waited for)
    ExportSeg *tab = reinterpret_cast<ExportSeg *>(d->export_tab.host.p);
    uint64_t units = 0;
    const bool iq = !F.real();
    const uint32_t rows = export_table(n_captures, m.data(), iq ? nullptr : p_hi.data(), at, out, iq ? kExportIqGroup : kExportPass, tab, &units);
    HIP_TRY(d, hipMemcpyAsync(d->export_tab.dev, d->export_tab.host, ((size_t)rows + 1) * sizeof(ExportSeg), hipMemcpyHostToDevice, st));
    const ExportSeg *tab_d = reinterpret_cast<const ExportSeg *>(d->export_tab.dev.p);
    if (iq)
        HIP_TRY(d, launch_iq_power_export_batch(tab_d, rows, units, st));
    else
        HIP_TRY(d, launch_power_export_batch(tab_d, rows, units, st));
    return (long)total;
}

// A batch in device memory: the checks, what the flavour puts in front (decoder_stage.hip: one launch, and a conversion's samples in
// the format report), the export launch behind it on the scan stream, and the wait -- also where the batch has no power sample to
// launch for: the scratch and the tables are the next call's to rewrite.
long export_batch(adsb_decoder *d, const char *what, const Flavour &F, size_t n_captures, const void *const *src, const size_t *n,
                  float *const *out, const size_t *cap)
{
    if (export_batch_refusal(d, what, F, true, n_captures, src, n, out, cap))
        return -1;
    HIP_TRY(d, hipSetDevice(d->device));
    std::vector<const void *> at;
    if (flavour_batch_to_scratch(d, what, F, n_captures, src, n, at))
        return -1;
    const long k = export_batch_launch(d, F, n_captures, at.data(), n, out, d->stream);
    if (k < 0)
        return -1;
    WAIT_STREAM(d, d->stream, "the scan stream");
    return k;
}

} // namespace

extern "C" {

long adsb_power_batch_device(adsb_decoder *d, size_t n_captures, const void *const *device_samples, const size_t *n,
                             float *const *device_power, const size_t *power_cap)
{
    return d ? export_batch(d, "adsb_power_batch_device", flavour_uint16(), n_captures, device_samples, n, device_power, power_cap) : -1;
}

long adsb_power_batch_device_as(adsb_decoder *d, int fmt, size_t n_captures, const void *const *device_samples, const size_t *n,
                                float *const *device_power, const size_t *power_cap)
{
    const char *what = "adsb_power_batch_device_as";
    Flavour F;
    if (!d)
        return -1;
    const int k = flavour_as(d, what, fmt, &F);
    if (k < 0)
        return -1;
    if (k)
        return adsb_power_batch_device(d, n_captures, device_samples, n, device_power, power_cap);
    return export_batch(d, what, F, n_captures, device_samples, n, device_power, power_cap);
}

long adsb_power_batch_device_packed(adsb_decoder *d, size_t n_captures, const void *const *device_packed, const size_t *n,
                                    float *const *device_power, const size_t *power_cap)
{
    return d ? export_batch(d, "adsb_power_batch_device_packed", flavour_packed(), n_captures, device_packed, n, device_power, power_cap) : -1;
}

long adsb_power_batch_device_iq(adsb_decoder *d, int fmt, size_t n_captures, const void *const *device_samples, const size_t *n,
                                float *const *device_power, const size_t *power_cap)
{
    const char *what = "adsb_power_batch_device_iq";
    Flavour F;
    if (!d)
        return -1;
    if (fmt == kFmtInt8Iq) // (the single call's refusal, word for word: decoder_export.hip)
        return d->fail("%s: format 8 (INT8_IQ) is not exported: the power export takes fmt 0 FLOAT32_IQ and 2 INT16_IQ only", what);
    if (flavour_iq(d, what, fmt, &F))
        return -1;
    return export_batch(d, what, F, n_captures, device_samples, n, device_power, power_cap);
}

long adsb_power_batch_host(adsb_decoder *d, size_t n_captures, const uint16_t *const *samples, const size_t *n, float *const *power,
                           const size_t *power_cap)
{
    const char *what = "adsb_power_batch_host";
    if (!d)
        return -1;
    const void *const *src = reinterpret_cast<const void *const *>(samples);
    if (export_batch_refusal(d, what, flavour_uint16().on_host(), false, n_captures, src, n, power, power_cap))
        return -1;
    HIP_TRY(d, hipSetDevice(d->device));
    // every capture at a 128-byte boundary of the scratch adsb_decode_batch_host lands its captures in, every capture's power
    // samples at a 128-byte boundary of adsb_power_window_host's; copies in, launch and copies out on ONE copy stream, in order
    // (a capture without a power sample takes no room in either)
    std::vector<size_t> in_bytes(n_captures), floats(n_captures);
    size_t all = 0;
    for (size_t i = 0; i < n_captures; i++) {
        floats[i] = (size_t)power_samples_produced(n[i]);
        in_bytes[i] = floats[i] ? n[i] * sizeof(uint16_t) : 0;
        all += floats[i];
    }
    if (all == 0)
        return 0;
    hipStream_t cs = d->copy_stream[0];
    std::vector<const void *> at;
    std::vector<float *> out;
    if (pow_slots(d, n_captures, floats.data(), out) ||
        land_captures(d, what, d->batch_in, "the captures", n_captures, src, in_bytes.data(), 128, Land::FirstCopyStream, at))
        return -1;
    const long r = export_batch_launch(d, flavour_uint16(), n_captures, at.data(), n, out.data(), cs);
    if (r < 0 || pow_slots_out(d, n_captures, power, out, floats.data(), cs))
        return -1;
    WAIT_STREAM(d, cs, "a copy stream");
    return r;
}

} // extern "C"
