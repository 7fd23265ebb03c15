// decoder_stage.hip -- the staging steps: a call's samples to where, and in the form, its kernel reads them.  Each step is written
// once here and called by every family (pushes, batch decodes, exports, levels; decoder_state.hpp names the buffers):
//   to_scratch        one capture in device memory -> uint16 / int16 in `unpacked`, by the unpack or a conversion on the scan stream
//   flavour_to_scratch / flavour_batch_to_scratch   ... what a flavour (flavour.hpp) puts in front of a kernel, one capture | a batch
//   land_captures     a batch's host captures -> batch_in or batch_land, side by side (stage_layout.hpp)
//   batch_to_scratch  a batch in device memory -> batch_unpacked by ONE unpack or conversion launch on the scan stream
//   window_in / floats_out   one host window -> win_buf; floats of pow_buf -> the caller's array
//   pow_slots / pow_slots_out   a batch's floats in pow_buf, each at a 32-float boundary, and back
// The rules they keep.  Streams: a step enqueues on the stream it names and waits only where it says so.  Alignment: 128 bytes for
// what a scan, export or level kernel reads (batch_in, batch_unpacked, uint16 / IQ / power landings), 16 bytes for what only the
// unpack or a conversion reads (the _as and packed landings), 64 Ki elements of rounding for win_buf and pow_buf.  Counters: a
// conversion adds its samples to fmt_converted and marks fmt_dirty; an unpack counts nothing; what is not converted is not counted.
// No kernel lives here.
#include "decoder_state.hpp"
#include "stage_layout.hpp"

using namespace adsb;

namespace {

constexpr size_t kWindowRound = 65535; // win_buf, pow_buf and the one-stream landings grow in steps of 64 Ki elements

// Room in a device scratch buffer of the handle's.
template <class T> int batch_grow(adsb_decoder *d, const char *what, const char *of, adsb::Buf<T> &buf, size_t bytes)
{
    if (buf.reserve(bytes / sizeof(T)) == hipSuccess)
        return 0;
    (void)hipGetLastError();
    return d->fail("%s: cannot allocate %zu bytes of device scratch for %s", what, bytes, of);
}

} // namespace

// conv = 0: the n samples (whole groups) of packed 12-bit input at src; else n elements of the conversion `conv`
// (sample_format.h) -> n uint16 in d->unpacked, enqueued on the scan stream and not waited for.  Every earlier use of the scratch
// has completed: the calls that use it return behind its reads.
int adsb::to_scratch(adsb_decoder *d, const char *what, int conv, const void *src, size_t n)
{
    HIP_TRY(d, hipSetDevice(d->device));
    if (d->unpacked.reserve(n) != hipSuccess) {
        (void)hipGetLastError();
        return d->fail("%s: cannot allocate %zu bytes of device scratch (2 bytes per sample)", what, n * sizeof(uint16_t));
    }
    if (!conv) {
        HIP_TRY(d, launch_unpack12(d->unpacked, src, n / kPackedGroupSamples, d->stream));
        return 0;
    }
    if (format_prepare(d, what, 0))
        return -1;
    HIP_TRY(d, launch_convert(conv, d->unpacked, src, n, d->d_fmt, d->stream));
    d->fmt_converted += n;
    d->fmt_dirty = true;
    return 0;
}

// What the flavour F puts in front of the kernel that reads ONE capture of n at src, which has a power sample (the callers return
// before): nothing, the unpack, or the conversion of F.scratch_elements(n) elements.  Returns what the kernel reads -- src itself, or
// d->unpacked -- or NULL: failed.
const void *adsb::flavour_to_scratch(adsb_decoder *d, const char *what, const Flavour &F, const void *src, size_t n)
{
    if (F.front == Flavour::kNone)
        return src;
    return to_scratch(d, what, F.conv, src, F.scratch_elements(n)) ? nullptr : d->unpacked.p;
}

// The in-place launches of a device push alternate onto the second scan stream, which nothing else orders behind to_scratch.
int adsb::scratch_before_stream2(adsb_decoder *d)
{
    if (!d->stream2)
        return 0;
    if (!d->ev_unpack)
        HIP_TRY(d, d->ev_unpack.create(hipEventDisableTiming));
    HIP_TRY(d, hipEventRecord(d->ev_unpack, d->stream));
    HIP_TRY(d, hipStreamWaitEvent(d->stream2, d->ev_unpack, 0));
    return 0;
}

// The host captures at src[] (bytes[i] each; 0: nothing to copy) -> buf, capture i at at[i], a multiple of `align` bytes.
// Land::InTurnWaited: copied on the copy streams in turn and all of them waited for -- the captures are the caller's again, and
// what reads them next needs no event; a failure to grow names `of`.  Land::FirstCopyStream: copied on copy_stream[0] in order and
// not waited for (what reads them is enqueued behind them on that stream); buf grows in steps of 64 Ki, as the window buffers do.
int adsb::land_captures(adsb_decoder *d, const char *what, adsb::Buf<uint8_t> &buf, const char *of, size_t n_captures, const void *const *src,
                        const size_t *bytes, size_t align, Land how, std::vector<const void *> &at)
{
    std::vector<size_t> off(n_captures);
    const size_t total = stage_layout(n_captures, bytes, align, off.data());
    if (how == Land::FirstCopyStream)
        HIP_TRY(d, buf.reserve((total + kWindowRound) & ~kWindowRound));
    else if (batch_grow(d, what, of, buf, total))
        return -1;
    at.resize(n_captures);
    for (size_t i = 0; i < n_captures; i++) {
        at[i] = buf + off[i];
        if (bytes[i])
            HIP_TRY(d, hipMemcpyAsync(buf + off[i], src[i], bytes[i], hipMemcpyHostToDevice,
                                      d->copy_stream[how == Land::FirstCopyStream ? 0 : i % adsb_decoder::kCopyStreams]));
    }
    if (how == Land::InTurnWaited)
        for (hipStream_t cs : d->copy_stream)
            WAIT_STREAM(d, cs, "a copy stream");
    return 0;
}

// The captures in device memory at src[] -- conv = 0: packed, n[i] samples in whole groups, 4-byte aligned; else n[i] elements of
// the conversion `conv`, aligned to the element -> uint16 in batch_unpacked, capture i from at[i] on (a 128-byte boundary), by ONE
// launch on the scan stream: what follows on that stream reads behind it.  Not waited for.  A conversion adds the batch's samples
// to the format report.  batch_unpacked_at: what adsb_batch_unpacked_copy answers from.
int adsb::batch_to_scratch(adsb_decoder *d, const char *what, int conv, size_t n_captures, const void *const *src, const size_t *n,
                           std::vector<const void *> &at)
{
    at.assign(n_captures, nullptr);
    d->batch_unpacked_at.clear();
    std::vector<size_t> bytes(n_captures), off(n_captures);
    size_t rows = 0, samples = 0;
    for (size_t i = 0; i < n_captures; i++) {
        bytes[i] = n[i] * sizeof(uint16_t);
        rows += n[i] != 0;
        samples += n[i];
    }
    const size_t total = stage_layout(n_captures, bytes.data(), 128, off.data());
    if (batch_grow(d, what, conv ? "the converted samples (2 bytes per sample)" : "the unpacked samples (2 bytes per sample)", d->batch_unpacked, total) ||
        (conv && format_prepare(d, what, 0)))
        return -1;
    const size_t tab_bytes = (rows + 1) * (conv ? sizeof(ConvertSeg) : sizeof(Unpack12Seg));
    HIP_TRY(d, d->unpack_tab.reserve(tab_bytes));
    for (size_t i = 0; i < n_captures; i++) {
        at[i] = reinterpret_cast<const char *>(d->batch_unpacked.p) + off[i];
        d->batch_unpacked_at.push_back(off[i] / sizeof(uint16_t));
    }
    d->batch_unpacked_at.push_back(total / sizeof(uint16_t));
    uint64_t groups = 0;
    const uint32_t n_rows = conv ? convert_table(n_captures, src, n, off.data(), reinterpret_cast<ConvertSeg *>(d->unpack_tab.host.p), &groups)
                                 : unpack12_table(n_captures, src, n, off.data(), reinterpret_cast<Unpack12Seg *>(d->unpack_tab.host.p), &groups);
    if (groups == 0)
        return 0;
    HIP_TRY(d, hipMemcpyAsync(d->unpack_tab.dev, d->unpack_tab.host, tab_bytes, hipMemcpyHostToDevice, d->stream));
    if (!conv) {
        HIP_TRY(d, launch_unpack12_batch(d->batch_unpacked, reinterpret_cast<const Unpack12Seg *>(d->unpack_tab.dev.p), n_rows, groups, d->stream));
        return 0;
    }
    HIP_TRY(d, launch_convert_batch(conv, d->batch_unpacked, reinterpret_cast<const ConvertSeg *>(d->unpack_tab.dev.p), n_rows, groups, d->d_fmt,
                                    d->stream));
    d->fmt_converted += samples;
    d->fmt_dirty = true;
    return 0;
}

// ... of a batch: at[i] is where the kernel reads capture i -- src[i] itself (and nothing of the handle changes), or its place in
// batch_unpacked behind the ONE launch of batch_to_scratch.  The two rules every operation keeps are Flavour::scratch_elements': a
// capture without a power sample is not converted and not counted; complex float32 samples are converted as 2 n scalars.
int adsb::flavour_batch_to_scratch(adsb_decoder *d, const char *what, const Flavour &F, size_t n_captures, const void *const *src, const size_t *n,
                                   std::vector<const void *> &at)
{
    if (F.front == Flavour::kNone) {
        at.assign(src, src + n_captures);
        return 0;
    }
    std::vector<size_t> sized(n_captures);
    for (size_t i = 0; i < n_captures; i++)
        sized[i] = F.scratch_elements(n[i]);
    return batch_to_scratch(d, what, F.conv, n_captures, src, sized.data(), at);
}

// The captures in device memory at at[] (bytes[i] each) that are not 16-byte aligned -> copies in batch_unpacked, each at a 128-byte
// boundary, by copies on the scan stream; at[i] then names the copy.  Not waited for.
int adsb::batch_realign(adsb_decoder *d, const char *what, size_t n_captures, const size_t *bytes, std::vector<const void *> &at)
{
    std::vector<size_t> moved(n_captures), off(n_captures);
    for (size_t i = 0; i < n_captures; i++)
        moved[i] = (uintptr_t)at[i] % 16 ? bytes[i] : 0;
    const size_t total = stage_layout(n_captures, moved.data(), 128, off.data());
    if (total && batch_grow(d, what, "the captures that are not 16-byte aligned", d->batch_unpacked, total))
        return -1;
    for (size_t i = 0; i < n_captures; i++) {
        if ((uintptr_t)at[i] % 16 == 0)
            continue;
        const void *from = at[i];
        at[i] = reinterpret_cast<const char *>(d->batch_unpacked.p) + off[i];
        if (bytes[i])
            HIP_TRY(d, hipMemcpyAsync(const_cast<void *>(at[i]), from, bytes[i], hipMemcpyDeviceToDevice, d->stream));
    }
    return 0;
}

// The caller's n uint16 samples -> win_buf, on the first copy stream and waited for: the launches that read the window may go to
// either compute stream.  floats > 0: room for as many floats in pow_buf too.
int adsb::window_in(adsb_decoder *d, const uint16_t *samples, size_t n, size_t floats)
{
    HIP_TRY(d, hipSetDevice(d->device));
    HIP_TRY(d, d->win_buf.reserve((n + kWindowRound) & ~kWindowRound));
    if (floats)
        HIP_TRY(d, d->pow_buf.reserve((floats + kWindowRound) & ~kWindowRound));
    HIP_TRY(d, hipMemcpyAsync(d->win_buf, samples, n * sizeof(uint16_t), hipMemcpyHostToDevice, d->copy_stream[0]));
    WAIT_STREAM(d, d->copy_stream[0], "a copy stream");
    return 0;
}

// The first `floats` floats of pow_buf -> dst in host memory, on the first copy stream and waited for (what wrote them has been).
int adsb::floats_out(adsb_decoder *d, float *dst, size_t floats)
{
    HIP_TRY(d, hipMemcpyAsync(dst, d->pow_buf, floats * sizeof(float), hipMemcpyDeviceToHost, d->copy_stream[0]));
    WAIT_STREAM(d, d->copy_stream[0], "a copy stream");
    return 0;
}

// Room in pow_buf for floats[i] floats per capture, each at a 32-float (128-byte) boundary: at[i], or NULL where floats[i] = 0.
int adsb::pow_slots(adsb_decoder *d, size_t n_captures, const size_t *floats, std::vector<float *> &at)
{
    std::vector<size_t> bytes(n_captures), off(n_captures);
    for (size_t i = 0; i < n_captures; i++)
        bytes[i] = floats[i] * sizeof(float);
    const size_t total = stage_layout(n_captures, bytes.data(), 128, off.data()) / sizeof(float);
    HIP_TRY(d, d->pow_buf.reserve((total + kWindowRound) & ~kWindowRound));
    at.resize(n_captures);
    for (size_t i = 0; i < n_captures; i++)
        at[i] = floats[i] ? d->pow_buf + off[i] / sizeof(float) : nullptr;
    return 0;
}

// ... and back: capture i's floats[i] floats from at[i] to dst[i] in host memory, on `st` behind what writes them; not waited for.
int adsb::pow_slots_out(adsb_decoder *d, size_t n_captures, float *const *dst, const std::vector<float *> &at, const size_t *floats, hipStream_t st)
{
    for (size_t i = 0; i < n_captures; i++)
        if (floats[i])
            HIP_TRY(d, hipMemcpyAsync(dst[i], at[i], floats[i] * sizeof(float), hipMemcpyDeviceToHost, st));
    return 0;
}

// What the batch exports and the batch level calls ask of capture i's samples, in this order and these words (the batch decodes word
// two of them differently: decoder_batch.hip batch_refusal).  Real samples end below 2^32 (the bound of complex and power samples is
// worded per family, by the caller).
int adsb::batch_samples_refusal(adsb_decoder *d, const char *what, size_t i, const void *src, size_t n, const Flavour &F)
{
    if (F.real() && (uint64_t)n >= (1ull << 32))
        return d->fail("%s: capture %zu has %zu samples: 2^32 or more, where the reference's sample counter wraps (air.c:34); "
                       "a batch has no long-stream mode", what, i, n);
    if (F.groups8 && n % kPackedGroupSamples != 0)
        return d->fail("%s: capture %zu: n = %zu is not a multiple of 8 (packed samples come in groups of 8 in 12 bytes)", what, i, n);
    if (F.in_align && (uintptr_t)src % F.in_align != 0)
        return d->fail("%s: capture %zu: device pointer %p is not %u-byte aligned", what, i, src, F.in_align);
    return 0;
}
