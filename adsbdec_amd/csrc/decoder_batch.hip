// decoder_batch.hip -- a batch of independent captures in as few launches as they fit (adsb_decode_batch_*, batch.hpp): the
// launches borrow a scan slot of the handle's (decoder_state.hpp) and are waited for one by one.
#include "decoder_state.hpp"

using namespace adsb;

namespace {

static_assert(adsb::kBatchRun == adsb::kRun && adsb::batch_tile_offsets(2) == (uint64_t)adsb::tile_offsets(2) &&
                  adsb::batch_tile_offsets(adsb::kMaxPasses) == (uint64_t)adsb::tile_offsets(adsb::kMaxPasses) &&
                  adsb::kBatchMaxLaunchOffsets == adsb::kMaxLaunchOffsets,
              "batch.hpp restates the tile geometry of scan_kernel.h");

int batch_passes_cap(uint64_t n_offsets, void *cus) { return adsb::choose_passes(n_offsets, *static_cast<int *>(cus)); }

inline int batch_forced_passes(int passes) { return (passes >= 2 && passes <= adsb::kMaxPasses) ? passes : 0; }

inline uint64_t batch_wanted_limit(int32_t knob) { return knob > 0 ? (uint64_t)knob : 0; } // (batch_launch_limit judges it)

// What every adsb_decode_batch_* call asks of its two arrays, first.
int batch_arrays_refusal(adsb_decoder *d, const char *what, size_t n_captures, const void *const *p, const size_t *n)
{
    return n_captures && (!p || !n) ? d->fail("%s: NULL capture arrays", what) : 0;
}

// The complex or power captures of a batch (n[] counts those samples): what a stream of the kind asks (flavour.hpp), per capture.
int batch_refusal_twos(adsb_decoder *d, const char *what, const Flavour &F, size_t n_captures, const void *const *p, const size_t *n)
{
    if (d->long_stream)
        return kind_refusal(d, what, F.kind);
    char who[96];
    for (size_t i = 0; i < n_captures; i++) {
        snprintf(who, sizeof who, "%s: capture %zu", what, i);
        if (units_refusal(d, who, F, p[i], n[i], 0))
            return -1;
    }
    return 0;
}

// The refusals of adsb_decode_batch_*, before anything of the handle changes, of the flavour F's captures (F.in_align = 0: in host
// memory).
int batch_refusal(adsb_decoder *d, const char *what, const Flavour &F, size_t n_captures, const void *const *p, const size_t *n)
{
    if (batch_arrays_refusal(d, what, n_captures, p, n))
        return -1;
    if (!F.real())
        return batch_refusal_twos(d, what, F, n_captures, p, n);
    for (size_t i = 0; i < n_captures; i++) {
        if ((uint64_t)n[i] >= (1ull << 32))
            return d->fail("%s: capture %zu has %zu samples: 2^32 or more, where the reference's sample counter wraps (air.c:34); "
                           "a batch has no long-stream mode", what, i, n[i]);
        if (F.groups8 && n[i] % adsb::kPackedGroupSamples != 0)
            return d->fail("%s: capture %zu: n = %zu is not a multiple of 8 (packed 12-bit input comes in whole 8-sample groups)", what,
                           i, n[i]);
        if (n[i] && !p[i])
            return d->fail("%s: capture %zu: NULL samples", what, i);
        if (F.in_align && (uintptr_t)p[i] % F.in_align != 0)
            return d->fail("%s: capture %zu: device pointer %p is not %u-byte aligned", what, i, p[i], F.in_align);
    }
    return 0;
}

// One launch of the batch: table up, scan, wait, regrow and repeat on overflow (by slot_collect's steps), then the sorted
// records and tries behind d->batch_cands / batch_tries, in virtual offsets.
int batch_launch_collect(adsb_decoder *d, const adsb_batch_launch &L, const void *const *p, const size_t *n)
{
    using clk = std::chrono::steady_clock;
    if (L.tiles == 0)
        return 0;
    const bool stats = d->cfg.collect_stats != 0;
    ScanSlot &s = d->slots[d->slot_head];
    uint64_t offsets = 0;
    uint32_t n_tab = 0; // segments with tiles
    for (uint32_t k = L.seg_first; k < L.seg_end; k++) {
        offsets += d->batch_segs[k].o_end - d->batch_segs[k].o_begin;
        n_tab += d->batch_segs[k].tiles != 0;
    }
    size_t cand_want, try_want;
    scan_record_room(d, offsets, &cand_want, &try_want);
    if (slot_reserve(d, s, std::max(s.cand_cap, cand_want), stats ? std::max(s.tries.cap, try_want) : s.tries.cap))
        return -1;
    // the table: the segments that have tiles, then a word per tile
    const size_t tab_bytes = (size_t)n_tab * sizeof(adsb::BatchSeg) + (size_t)L.tiles * sizeof(uint32_t);
    HIP_TRY(d, d->batch_tab.reserve(tab_bytes));
    adsb::BatchSeg *seg_h = reinterpret_cast<adsb::BatchSeg *>(d->batch_tab.host.p);
    uint32_t *tile_h = reinterpret_cast<uint32_t *>(seg_h + n_tab);
    uint32_t row = 0;
    for (uint32_t k = L.seg_first; k < L.seg_end; k++) {
        const adsb_batch_segment &sg = d->batch_segs[k];
        if (sg.tiles == 0)
            continue;
        // in the launch's coordinates the capture's pair 0 is pair `origin`: the buffer holds pairs from there on, and nothing
        // below it exists (a stream's start: silence, air.c:33)
        const int64_t origin = (int64_t)(sg.base - L.g_begin) - (int64_t)sg.o_begin;
        adsb::BatchSeg &b = seg_h[row];
        b.x = (uint64_t)(uintptr_t)p[sg.capture];
        b.pbuf0 = origin;
        b.p_lo = origin;
        // (flush: the silent twin ends at the capture's last whole quad; the pair of a trailing partial one reads as silence too)
        b.p_hi = origin + (int64_t)(d->flush ? adsb::batch_power_flush(n[sg.capture]) : n[sg.capture] / 2);
        b.g_begin = sg.base - L.g_begin;
        b.g_end = b.g_begin + (sg.o_end - sg.o_begin);
        b.first_tile = sg.first_tile;
        b.pad = 0;
        for (uint32_t t = 0; t < sg.tiles; t++)
            tile_h[sg.first_tile + t] = row;
        row++;
    }
    hipStream_t ls = d->stream;
    HIP_TRY(d, hipMemcpyAsync(d->batch_tab.dev, d->batch_tab.host, tab_bytes, hipMemcpyHostToDevice, ls));
    const adsb::BatchSeg *seg_d = reinterpret_cast<const adsb::BatchSeg *>(d->batch_tab.dev.p);
    const uint32_t *tile_d = reinterpret_cast<const uint32_t *>(seg_d + n_tab);

    adsb::ScanArgs &a = s.args;
    a = adsb::ScanArgs{};
    a.g_begin = 0; // the launch's own coordinates: g_rel = virtual offset - L.g_begin
    a.g_end = L.g_end - L.g_begin;
    fill_scan_args(d, a);
    a.passes = L.passes;
    a.big_tiles = 0;
    s.streaming = false;
    s.tries_on_device = s.try_regions = false;
    s.epoch_base = 0;
    s.ntiles = L.tiles;
    if (slot_order_behind_count(d, s, ls)) // (as slot_launch: what may still use the slot's past)
        return -1;
    const auto t_wait = clk::now();
    // (slot_collect's loop -- await_counters -- waits for a launch that is in flight and relaunches through slot_launch; this one
    // launches itself, every time round, and waits at once: the two share their steps, not the loop)
    for (int attempt = 0;; attempt++) {
        if (slot_begin_launch(d, s, ls, offsets))
            return -1;
        a.tries = s.tries;
        a.try_cap = (uint32_t)std::min<size_t>(s.tries.cap, 0xFFFFFFFFu);
        s.busy = true; // (a failure from here on leaves a launch in flight: adsb_reset waits for it)
        if (d->kind == adsb::kKindIq)
            HIP_TRY(d, adsb::launch_scan_batch_iq(a, seg_d, tile_d, L.tiles, stats, ls));
        else if (d->kind == adsb::kKindIq8)
            HIP_TRY(d, adsb::launch_scan_batch_iq8(a, seg_d, tile_d, L.tiles, stats, ls));
        else if (d->kind == adsb::kKindPower)
            HIP_TRY(d, adsb::launch_scan_batch_power(a, seg_d, tile_d, L.tiles, stats, ls));
        else
            HIP_TRY(d, adsb::launch_scan_batch(a, seg_d, tile_d, L.tiles, stats, ls));
        HIP_TRY(d, hipEventRecord(s.ev_ready[s.ev_cur], ls));
        WAIT_EVENT(d, s.ev_ready[s.ev_cur], "a batch scan launch");
        s.busy = false;
        book_launch(d, s, offsets);
        if (slot_settle_profile(d, s, s.ev_cur))
            return -1;
        const int again = regrow_if_overflowed(d, s, attempt); // (the stream it waits for first is idle here)
        if (again < 0)
            return -1;
        if (!again)
            break;
    }
    const auto t_host = clk::now();
    d->prof.wait_ms += std::chrono::duration<double, std::milli>(t_host - t_wait).count();
    const size_t nc = s.hc()[0], nt = s.hc()[1];
    sort_order(d, s.cands, nc);
    if (nt)
        sort_tries(d, s.tries, nt);
    d->prof.candidates += nc;
    d->prof.tries += nt;
    const size_t at = d->batch_cands.size();
    d->batch_cands.resize(at + nc);
    for (size_t i = 0; i < nc; i++)
        d->batch_cands[at + i] = adsb::record_candidate(s.cands + (size_t)d->order[i] * adsb::kCandWords, L.g_begin);
    const size_t tat = d->batch_tries.size();
    d->batch_tries.resize(tat + nt);
    for (size_t i = 0; i < nt; i++)
        d->batch_tries[tat + i] = (((uint64_t)(s.tries[i] >> 2) + L.g_begin) << 2) | (s.tries[i] & 3u);
    d->prof.host_ms += std::chrono::duration<double, std::milli>(clk::now() - t_host).count();
    return 0;
}

long decode_batch(adsb_decoder *d, size_t n_captures, const void *const *p, const size_t *n, const adsb_frame **frames,
                  uint64_t *first, adsb_stats *stats)
{
    using clk = std::chrono::steady_clock;
    size_t bad = 0;
    // A batch is whole streams, ended: like adsb_decode_device it leaves the handle finished, whether it succeeds or not,
    // so a push without adsb_reset is refused and never meets batch_stats or the batch's frames.
    d->finished = true;
    if (!adsb::batch_layout(n_captures, n, batch_passes_cap, &d->n_cus, batch_forced_passes(d->dbg.passes),
                            batch_wanted_limit(d->dbg.batch_launch_offsets), d->batch_segs, d->batch_launches, &bad, d->flush))
        return d->fail("internal: capture %zu is too long for a batch", bad); // (batch_refusal has looked)
    d->batch_cands.clear();
    d->batch_tries.clear();
    for (const adsb_batch_launch &L : d->batch_launches)
        if (batch_launch_collect(d, L, p, n))
            return -1;
    const auto t_host = clk::now();
    d->batch_per.resize(n_captures); // every capture's table: the caller's `stats`, and the sum adsb_get_stats answers
    const bool ok = adsb::batch_resolve(d->batch_res, n_captures, n, d->batch_segs.data(), d->batch_segs.size(), d->batch_cands.data(),
                                        d->batch_cands.size(), d->batch_tries.data(), d->batch_tries.size(), d->batch_frames, first,
                                        d->batch_per.data(), d->batch_cbuf, d->batch_tbuf, d->flush);
    if (!ok) {
        d->batch_frames.clear();
        return d->fail("internal: a record of a batch launch lies in no capture's offsets");
    }
    std::memset(&d->batch_stats, 0, sizeof d->batch_stats);
    for (size_t i = 0; i < n_captures; i++) {
        const adsb_stats &st = d->batch_per[i];
        for (int k = 0; k < 3; k++) {
            d->batch_stats.try_[k] += st.try_[k];
            d->batch_stats.ok[k] += st.ok[k];
        }
        d->batch_stats.fixed += st.fixed;
        if (stats)
            stats[i] = st;
    }
    d->batch_stats_on = true;
    d->prof.host_ms += std::chrono::duration<double, std::milli>(clk::now() - t_host).count();
    *frames = d->batch_frames.empty() ? nullptr : d->batch_frames.data();
    return (long)d->batch_frames.size();
}


// Unpack or convert, decode; and the stream idle behind it whatever the result (a batch without an offset launches no scan that would
// have been waited for: the table and the scratch are the next call's to rewrite).  Every sample goes through the launch in front, not
// Flavour::scratch_elements' choice: a decode reads a capture's trailing partial quad too.
long decode_batch_front(adsb_decoder *d, const char *what, const Flavour &F, size_t n_captures, const void *const *src, const size_t *n,
                        const adsb_frame **frames, uint64_t *first, adsb_stats *stats)
{
    std::vector<const void *> at;
    d->finished = true; // (as decode_batch: a failure from here on leaves a finished handle too)
    if (batch_to_scratch(d, what, F.conv, n_captures, src, n, at))
        return -1;
    const long k = decode_batch(d, n_captures, at.data(), n, frames, first, stats);
    WAIT_STREAM(d, d->stream, "the scan stream");
    return k;
}

// ---- batches of IQ and float32 power captures (adsb_decode_batch_*_iq, _power) ----
// n[] counts complex or power samples.  The batch machinery counts 16-bit units and ends a capture by the real streams' rule (a
// trailing partial quad still yields two power samples); these captures' power samples enter in twos and a trailing odd one is never
// seen (air.c:94-99), which is exactly what the machinery does for the capture WITHOUT that sample: units[i] = 4 (n[i] / 2).
// The captures in device memory at src[] (int16 pairs or float32 power samples, 4-byte aligned; float pairs; int8 pairs, 2-byte
// aligned) -> frames.  Whatever is not 16-byte aligned int16 goes through scratch first: FLOAT32_IQ by the batch conversion launch, a
// misaligned capture of the others by a copy.  The layout is asked at the number the widened twin is asked at, 4 (n / 2), so
// segments, tiles and launches are the twin's; a unit of an int8 capture is a BYTE there (kind_unit_bytes), which only the scratch
// copies of the captures that are not 16-byte aligned see -- the segment table counts complex samples either way.
long decode_batch_twos(adsb_decoder *d, const char *what, const Flavour &F, size_t n_captures, const void *const *src, const size_t *n,
                       const adsb_frame **frames, uint64_t *first, adsb_stats *stats)
{
    std::vector<size_t> units(n_captures);
    for (size_t i = 0; i < n_captures; i++)
        units[i] = 4 * (n[i] / 2);
    std::vector<const void *> at;
    d->finished = true; // (as decode_batch: a failure from here on leaves a finished handle too)
    if (flavour_batch_to_scratch(d, what, F, n_captures, src, n, at))
        return -1;
    if (F.front == Flavour::kNone) {
        d->batch_unpacked_at.clear(); // (adsb_batch_unpacked_copy: no table of this call's; the copies rewrite the scratch)
        std::vector<size_t> bytes(n_captures);
        for (size_t i = 0; i < n_captures; i++)
            bytes[i] = units[i] * adsb::kind_unit_bytes(F.kind);
        if (batch_realign(d, what, n_captures, bytes.data(), at))
            return -1;
    }
    d->kind = F.kind; // (behind the reset: the batch launches are this kind's kernel's)
    const long k = decode_batch(d, n_captures, at.data(), units.data(), frames, first, stats);
    WAIT_STREAM(d, d->stream, "the scan stream");
    return k;
}

// The host captures of a batch (bytes_of(n[i]) bytes each) into `buf`, each at a multiple of `align` bytes: copied on the copy streams in
// turn and waited for -- the captures are the caller's again, and the unpack, conversion or scan that reads them needs no event.
template <class BytesOf>
int land_batch(adsb_decoder *d, const char *what, adsb::Buf<uint8_t> &buf, const char *of, size_t n_captures, const void *const *src,
               const size_t *n, BytesOf bytes_of, size_t align, std::vector<const void *> &at)
{
    std::vector<size_t> bytes(n_captures);
    for (size_t i = 0; i < n_captures; i++)
        bytes[i] = bytes_of(n[i]);
    return land_captures(d, what, buf, of, n_captures, src, bytes.data(), align, adsb::Land::InTurnWaited, at);
}

// every entry point behind its refusals: a fresh stream on the handle's device
int batch_begin(adsb_decoder *d)
{
    if (adsb_reset(d) != 0)
        return -1;
    HIP_TRY(d, hipSetDevice(d->device));
    return 0;
}

} // namespace

extern "C" {

long adsb_decode_batch_device_power(adsb_decoder *d, size_t n_captures, const void *const *device_samples, const size_t *n,
                                    const adsb_frame **frames, uint64_t *first, adsb_stats *stats)
{
    const char *what = "adsb_decode_batch_device_power";
    if (!d || !frames || !first)
        return -1;
    if (batch_refusal(d, what, flavour_power(), n_captures, device_samples, n) || batch_begin(d))
        return -1;
    return decode_batch_twos(d, what, flavour_power(), n_captures, device_samples, n, frames, first, stats);
}

long adsb_decode_batch_host_power(adsb_decoder *d, size_t n_captures, const float *const *samples, const size_t *n,
                                  const adsb_frame **frames, uint64_t *first, adsb_stats *stats)
{
    const char *what = "adsb_decode_batch_host_power";
    const void *const *src = reinterpret_cast<const void *const *>(samples);
    if (!d || !frames || !first)
        return -1;
    if (batch_refusal(d, what, flavour_power().on_host(), n_captures, src, n) || batch_begin(d))
        return -1;
    // every capture as it is at a 128-byte boundary of the landing buffer the other host batches use
    std::vector<const void *> land;
    if (land_batch(d, what, d->batch_land, "the captures as they are", n_captures, src, n, [](size_t k) { return k * sizeof(float); }, 128, land))
        return -1;
    return decode_batch_twos(d, what, flavour_power(), n_captures, land.data(), n, frames, first, stats);
}

long adsb_decode_batch_device_iq(adsb_decoder *d, int fmt, size_t n_captures, const void *const *device_samples, const size_t *n,
                                 const adsb_frame **frames, uint64_t *first, adsb_stats *stats)
{
    const char *what = "adsb_decode_batch_device_iq";
    Flavour F;
    if (!d || !frames || !first)
        return -1;
    if (batch_arrays_refusal(d, what, n_captures, device_samples, n) || flavour_iq(d, what, fmt, &F) ||
        batch_refusal(d, what, F, n_captures, device_samples, n) || batch_begin(d))
        return -1;
    return decode_batch_twos(d, what, F, n_captures, device_samples, n, frames, first, stats);
}

long adsb_decode_batch_host_iq(adsb_decoder *d, int fmt, size_t n_captures, const void *const *samples, const size_t *n,
                               const adsb_frame **frames, uint64_t *first, adsb_stats *stats)
{
    const char *what = "adsb_decode_batch_host_iq";
    Flavour F;
    if (!d || !frames || !first)
        return -1;
    if (batch_arrays_refusal(d, what, n_captures, samples, n) || flavour_iq(d, what, fmt, &F) ||
        batch_refusal(d, what, F.on_host(), n_captures, samples, n) || batch_begin(d))
        return -1;
    // every capture as it is at a 128-byte boundary of the landing buffer the other host batches use
    std::vector<const void *> land;
    const size_t elem = adsb::iq_sample_bytes(fmt);
    if (land_batch(d, what, d->batch_land, "the captures as they are", n_captures, samples, n, [elem](size_t k) { return k * elem; }, 128, land))
        return -1;
    return decode_batch_twos(d, what, F, n_captures, land.data(), n, frames, first, stats);
}

long adsb_decode_batch_device_as(adsb_decoder *d, int fmt, size_t n_captures, const void *const *device_samples, const size_t *n,
                                 const adsb_frame **frames, uint64_t *first, adsb_stats *stats)
{
    const char *what = "adsb_decode_batch_device_as";
    Flavour F;
    if (!d || !frames || !first)
        return -1;
    const int k = flavour_as(d, what, fmt, &F);
    if (k < 0)
        return -1;
    if (k)
        return adsb_decode_batch_device(d, n_captures, device_samples, n, frames, first, stats);
    if (batch_refusal(d, what, F, n_captures, device_samples, n) || batch_begin(d))
        return -1;
    return decode_batch_front(d, what, F, n_captures, device_samples, n, frames, first, stats);
}

long adsb_decode_batch_host_as(adsb_decoder *d, int fmt, size_t n_captures, const void *const *samples, const size_t *n,
                               const adsb_frame **frames, uint64_t *first, adsb_stats *stats)
{
    const char *what = "adsb_decode_batch_host_as";
    Flavour F;
    if (!d || !frames || !first)
        return -1;
    const int k = flavour_as(d, what, fmt, &F);
    if (k < 0)
        return -1;
    if (k)
        return adsb_decode_batch_host(d, n_captures, reinterpret_cast<const uint16_t *const *>(samples), n, frames, first, stats);
    if (batch_refusal(d, what, F.on_host(), n_captures, samples, n) || batch_begin(d))
        return -1;
    // every capture's samples at a 16-byte boundary of the landing buffer the packed batches use
    std::vector<const void *> land;
    const size_t elem = F.in_align; // (a converted format's alignment is its element)
    if (land_batch(d, what, d->batch_land, "the captures as they are", n_captures, samples, n, [elem](size_t k) { return k * elem; }, 16, land))
        return -1;
    return decode_batch_front(d, what, F, n_captures, land.data(), n, frames, first, stats);
}

long adsb_decode_batch_device(adsb_decoder *d, size_t n_captures, const void *const *device_samples, const size_t *n,
                              const adsb_frame **frames, uint64_t *first, adsb_stats *stats)
{
    if (!d || !frames || !first)
        return -1;
    if (batch_refusal(d, "adsb_decode_batch_device", flavour_uint16(), n_captures, device_samples, n) || batch_begin(d))
        return -1;
    d->batch_unpacked_at.clear(); // (adsb_batch_unpacked_copy: this call unpacks and converts nothing)
    return decode_batch(d, n_captures, device_samples, n, frames, first, stats);
}

long adsb_decode_batch_host(adsb_decoder *d, size_t n_captures, const uint16_t *const *samples, const size_t *n,
                            const adsb_frame **frames, uint64_t *first, adsb_stats *stats)
{
    const char *what = "adsb_decode_batch_host";
    const void *const *src = reinterpret_cast<const void *const *>(samples);
    if (!d || !frames || !first)
        return -1;
    if (batch_refusal(d, what, flavour_uint16().on_host(), n_captures, src, n) || batch_begin(d))
        return -1;
    // every capture at a 128-byte boundary of one scratch array of the handle's
    d->batch_unpacked_at.clear(); // (as adsb_decode_batch_device)
    std::vector<const void *> at;
    if (land_batch(d, what, d->batch_in, "the captures", n_captures, src, n, [](size_t k) { return k * sizeof(uint16_t); }, 128, at))
        return -1;
    return decode_batch(d, n_captures, at.data(), n, frames, first, stats);
}

long adsb_decode_batch_device_packed(adsb_decoder *d, size_t n_captures, const void *const *device_packed, const size_t *n,
                                     const adsb_frame **frames, uint64_t *first, adsb_stats *stats)
{
    const char *what = "adsb_decode_batch_device_packed";
    if (!d || !frames || !first)
        return -1;
    if (batch_refusal(d, what, flavour_packed(), n_captures, device_packed, n) || batch_begin(d))
        return -1;
    return decode_batch_front(d, what, flavour_packed(), n_captures, device_packed, n, frames, first, stats);
}

long adsb_decode_batch_host_packed(adsb_decoder *d, size_t n_captures, const void *const *packed, const size_t *n,
                                   const adsb_frame **frames, uint64_t *first, adsb_stats *stats)
{
    const char *what = "adsb_decode_batch_host_packed";
    if (!d || !frames || !first)
        return -1;
    if (batch_refusal(d, what, flavour_packed().on_host(), n_captures, packed, n) || batch_begin(d))
        return -1;
    // only the packed bytes cross the link: every capture's at a 16-byte boundary of one landing buffer of the handle's
    std::vector<const void *> land;
    if (land_batch(d, what, d->batch_land, "the packed captures (1.5 bytes per sample)", n_captures, packed, n,
                   [](size_t k) { return (size_t)ADSB_PACKED12_BYTES(k); }, 16, land))
        return -1;
    return decode_batch_front(d, what, flavour_packed(), n_captures, land.data(), n, frames, first, stats);
}

long adsb_batch_layout_flush(size_t n_captures, const size_t *n, int cus, int passes, uint64_t launch_offsets, int flush,
                             adsb_batch_segment *segs, size_t seg_cap, adsb_batch_launch *launches, size_t launch_cap, size_t *n_launches)
{
    if ((n_captures && !n) || (seg_cap && !segs) || (launch_cap && !launches) || !n_launches)
        return -1;
    std::vector<adsb_batch_segment> sv;
    std::vector<adsb_batch_launch> lv;
    if (!adsb::batch_layout(n_captures, n, batch_passes_cap, &cus, batch_forced_passes(passes), launch_offsets, sv, lv, nullptr, flush != 0))
        return -1;
    if (!sv.empty() && seg_cap)
        std::memcpy(segs, sv.data(), std::min(seg_cap, sv.size()) * sizeof sv[0]);
    if (!lv.empty() && launch_cap)
        std::memcpy(launches, lv.data(), std::min(launch_cap, lv.size()) * sizeof lv[0]);
    *n_launches = lv.size();
    return (long)sv.size();
}

long adsb_batch_layout_ex(size_t n_captures, const size_t *n, int cus, int passes, uint64_t launch_offsets, adsb_batch_segment *segs,
                          size_t seg_cap, adsb_batch_launch *launches, size_t launch_cap, size_t *n_launches)
{
    return adsb_batch_layout_flush(n_captures, n, cus, passes, launch_offsets, 0, segs, seg_cap, launches, launch_cap, n_launches);
}

long adsb_batch_layout(size_t n_captures, const size_t *n, int cus, int passes, adsb_batch_segment *segs, size_t seg_cap,
                       adsb_batch_launch *launches, size_t launch_cap, size_t *n_launches)
{
    return adsb_batch_layout_ex(n_captures, n, cus, passes, 0, segs, seg_cap, launches, launch_cap, n_launches);
}

long adsb_batch_resolve_flush(size_t n_captures, const size_t *n, int cus, int passes, uint64_t launch_offsets, int flush,
                              const adsb_candidate *cands, size_t n_cands, const uint64_t *tries, size_t n_tries, adsb_frame *frames,
                              size_t frame_cap, uint64_t *first, adsb_stats *stats)
{
    if ((n_captures && !n) || (n_cands && !cands) || (n_tries && !tries) || (frame_cap && !frames) || !first)
        return -1;
    std::vector<adsb_batch_segment> sv;
    std::vector<adsb_batch_launch> lv;
    if (!adsb::batch_layout(n_captures, n, batch_passes_cap, &cus, batch_forced_passes(passes), launch_offsets, sv, lv, nullptr, flush != 0))
        return -1;
    adsb::Resolver r;
    std::vector<adsb_frame> out;
    std::vector<adsb_candidate> cbuf;
    std::vector<uint64_t> tbuf;
    if (!adsb::batch_resolve(r, n_captures, n, sv.data(), sv.size(), cands, n_cands, tries, n_tries, out, first, stats, cbuf, tbuf, flush != 0))
        return -1;
    if (!out.empty() && out.size() <= frame_cap)
        std::memcpy(frames, out.data(), out.size() * sizeof out[0]);
    return (long)out.size();
}

long adsb_batch_resolve_ex(size_t n_captures, const size_t *n, int cus, int passes, uint64_t launch_offsets, const adsb_candidate *cands,
                           size_t n_cands, const uint64_t *tries, size_t n_tries, adsb_frame *frames, size_t frame_cap, uint64_t *first,
                           adsb_stats *stats)
{
    return adsb_batch_resolve_flush(n_captures, n, cus, passes, launch_offsets, 0, cands, n_cands, tries, n_tries, frames, frame_cap, first, stats);
}

long adsb_batch_resolve(size_t n_captures, const size_t *n, int cus, int passes, const adsb_candidate *cands, size_t n_cands,
                        const uint64_t *tries, size_t n_tries, adsb_frame *frames, size_t frame_cap, uint64_t *first, adsb_stats *stats)
{
    return adsb_batch_resolve_ex(n_captures, n, cus, passes, 0, cands, n_cands, tries, n_tries, frames, frame_cap, first, stats);
}

int adsb_batch_records(adsb_decoder *d, const adsb_candidate **cands, size_t *n_cands, const uint64_t **tries, size_t *n_tries,
                       const adsb_batch_segment **segs, size_t *n_segs, const adsb_batch_launch **launches, size_t *n_launches)
{
    if (!d)
        return -1;
    if (cands)
        *cands = d->batch_cands.data();
    if (n_cands)
        *n_cands = d->batch_cands.size();
    if (tries)
        *tries = d->batch_tries.data();
    if (n_tries)
        *n_tries = d->batch_tries.size();
    if (segs)
        *segs = d->batch_segs.data();
    if (n_segs)
        *n_segs = d->batch_segs.size();
    if (launches)
        *launches = d->batch_launches.data();
    if (n_launches)
        *n_launches = d->batch_launches.size();
    return 0;
}

int adsb_batch_unpacked_copy(adsb_decoder *d, size_t capture, uint16_t *dst_u16, size_t n)
{
    if (!d)
        return -1;
    // batch_unpacked_at: where every capture of the last packed or converted batch call starts in the scratch (samples), and where
    // the last one's slot ends; empty behind a batch call that fills no such table
    if (capture + 1 >= d->batch_unpacked_at.size())
        return d->fail("adsb_batch_unpacked_copy: the last packed or converted batch call had no capture %zu", capture);
    const size_t at = d->batch_unpacked_at[capture], slot = d->batch_unpacked_at[capture + 1] - at;
    if (n > slot)
        return d->fail("adsb_batch_unpacked_copy: capture %zu has a slot of %zu samples, %zu were asked for", capture, slot, n);
    if (n == 0)
        return 0;
    if (!dst_u16)
        return d->fail("adsb_batch_unpacked_copy: NULL destination");
    HIP_TRY(d, hipSetDevice(d->device));
    HIP_TRY(d, hipMemcpyAsync(dst_u16, d->batch_unpacked.p + at, n * sizeof(uint16_t), hipMemcpyDeviceToHost, d->stream));
    WAIT_STREAM(d, d->stream, "the copy of a batch's unpacked samples");
    return 0;
}

} // extern "C"
