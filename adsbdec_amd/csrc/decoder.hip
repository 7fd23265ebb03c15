// decoder.hip -- the stream machinery of libadsbdec_amd.so's host side: device staging, kernel launches, the count passes,
// and the C-ABI calls of include/adsbdec_amd.h that push, finish and read a stream.  What a launch leaves behind is collected
// in decoder_collect.hip; the handle itself and the units beside this one: decoder_state.hpp.
#include "decoder_state.hpp"
#include "packed12.h"
#include "sample_format.h"
#include "seam_kernel.h"

using namespace adsb;

namespace adsb {

// Offsets per launch.  With the streaming
// hand-off the host already overlaps a launch while it runs, so launches are as large
// as the record buffers sensibly allow (each launch carries ~20 us of ramp and tail);
// the collect-after-completion path needs several launches in flight to overlap at all.
static uint64_t chunk_offsets(bool streaming)
{
    static const uint64_t forced = [] {
        const char *e = tuning_env("ADSB_CHUNK_MI");
        const uint64_t mi = e ? strtoull(e, nullptr, 10) : 0;
        return (mi >= 1 && mi <= 512) ? mi : 0;
    }();
    const uint64_t mi = forced ? forced : (streaming ? 128 : 64);
    return 28ull * ((mi << 20) / 28);
}

// Where unit `unit` of staging buffer `buf` lies: the buffers are arrays of 16-bit units for every kind but an int8 IQ stream's,
// whose units are bytes (decoder_state.hpp kind_unit_bytes).
static inline uint16_t *stage_at(adsb_decoder *d, int buf, uint64_t unit)
{
    return reinterpret_cast<uint16_t *>(reinterpret_cast<char *>(d->stage[buf].p) + unit * adsb::kind_unit_bytes(d->kind));
}

// One past the last offset that can be scanned once `n_samples` samples of the stream are in: the whole 1196-sample
// window of an offset must have been produced.  A stream produces power samples in twos (air.c:59-92); a shard's samples
// end where its last owned window does (adsb_plan_shards), which need not be a whole quad, and its scan never goes
// beyond the offsets it owns.
static uint64_t scannable_end(const adsb_decoder *d, uint64_t n_samples, bool final)
{
    uint64_t m = power_samples_produced(n_samples);
    if (d->shard_on)
        m = n_samples / 2; // every complete pair
    uint64_t g_end = m >= ADSB_WINDOW ? m - ADSB_WINDOW + 1 : 0;
    if (final && d->flush && !d->shard_on)
        g_end = m; // flush: the last launch owns every offset of the stream; the windows behind the last power sample read silence
    if (!final && d->long_stream) {
        // run boundaries are those of the EPOCH (a scan launch is given epoch-relative indices, and 2^31 mod 28 = 16); a scan
        // may stop anywhere among the seam offsets of a wrap, which need no alignment -- only the staging tail's (4 offsets)
        const uint64_t P = round_down(g_end, adsb::kEpoch), r = g_end - P;
        const bool in_seam = (P && r < (uint64_t)adsb::kSeamBehind) || r >= adsb::kEpoch - adsb::kSeamWindow;
        g_end = in_seam ? round_down(g_end, 4) : P + round_down(r, 28);
    } else if (!final)
        g_end = round_down(g_end, 28);
    if (d->shard_on && g_end > d->shard_g_end)
        g_end = d->shard_g_end;
    return g_end;
}

// adsb_push_async: wait for the copy of the last piece (a no-op when a collected scan has implied it).
int wait_last_copy(adsb_decoder *d)
{
    if (d->piece == 0 || d->dbg_async == 2)
        return 0;
    HIP_TRY(d, hipSetDevice(d->device));
    WAIT_EVENT(d, d->ev_copy[d->piece % adsb_decoder::kCopyStreams], "the host-to-device copy of the previous piece");
    return 0;
}

// The reference's ring index `fidx` is a uint32_t that counts input samples (air.c:34): at 2^32 samples it
// wraps, 2^32 mod 14 = 4, and the ring phase jumps.  By default a stream is refused there; a handle with
// adsb_set_long_stream follows the reference through the wrap (scan_submit, seam_kernel.hip; DESIGN.md "Input domain").
bool stream_too_long(adsb_decoder *d, size_t n)
{
    if (d->long_stream || d->n_samples + (uint64_t)n < (1ull << 32))
        return false;
    d->fail("stream would reach 2^32 samples: the reference's sample counter wraps there (air.c:34); adsb_set_long_stream decodes beyond");
    return true;
}

// The same limit for the shard primitives, which take stream positions instead of counting pushes: a window
// [first_sample, first_sample + n) and a stream length total_samples must both stay below 2^32 samples.
bool shard_too_long(adsb_decoder *d, const char *what, uint64_t first_sample, uint64_t n, uint64_t total_samples)
{
    const uint64_t lim = 1ull << 32;
    if (first_sample < lim && n < lim - first_sample && total_samples < lim)
        return false;
    d->fail("%s: %s reaches 2^32 samples: the reference's sample counter wraps there (air.c:34) and no parity is defined beyond",
            what, total_samples < lim ? "window" : "stream");
    return true;
}

int slot_reserve_device_tries(adsb_decoder *d, ScanSlot &s, size_t want_list, size_t want_tiles)
{
    if (want_list > s.d_try_cap || want_tiles > s.d_try_tiles) {
        want_list = std::max(want_list, s.d_try_cap);
        want_tiles = std::max(want_tiles, s.d_try_tiles);
        if (d->count_stream) { // a count pass may still be reading the old arrays
            if (count_flush(d))
                return -1;
            WAIT_STREAM(d, d->count_stream, "the try-count stream");
        }
        s.d_try_cap = s.d_try_tiles = 0;
        HIP_TRY(d, s.d_tries.reserve(want_tiles * adsb::kTryRegion + want_list));
        HIP_TRY(d, s.d_try_counts.reserve(std::max<size_t>(want_tiles, 1)));
        s.d_try_cap = want_list;
        s.d_try_tiles = want_tiles;
    }
    return 0;
}

int slot_reserve(adsb_decoder *d, ScanSlot &s, size_t want_cands, size_t want_tries)
{
    if (want_cands > s.cand_cap) {
        s.cand_cap = 0;
        HIP_TRY(d, s.cands.reserve(want_cands * adsb::kCandWords));
        s.cand_cap = want_cands;
    }
    HIP_TRY(d, s.tries.reserve(want_tries));
    return 0;
}

// Kernel time of a collected launch (cfg.profile): the tiles leave the earliest start and
// the latest end of the device's 100 MHz clock in the counters -- no events, no extended
// launch.  Read lazily (behind the slot's next launch, or in adsb_get_profile): waiting for
// the counters right after the last tile has been consumed would put a device round trip on
// the critical path of every push.
int slot_settle_profile(adsb_decoder *d, ScanSlot &s, int copy)
{
    if (!s.prof_pending[copy])
        return 0;
    s.prof_pending[copy] = false;
    WAIT_EVENT(d, s.ev_ready[copy], "a scan launch");
    const uint32_t *c = s.h_counters + copy * adsb::kCounterWords;
    const uint64_t t_begin = ~((uint64_t)c[5] << 32 | c[4]), t_end = (uint64_t)c[7] << 32 | c[6];
    const double ms = t_end > t_begin ? (double)(t_end - t_begin) * 1e-5 : 0.0; // 10 ns ticks
    d->prof.kernel_ms += ms;
    d->prof.last_kernel_ms = ms;
    const uint64_t no = s.ev_offsets[copy];
    if (no > d->prof.big_offsets) {
        d->prof.big_offsets = no;
        d->prof.big_launches = 0;
        d->prof.big_ms = 0;
    }
    if (no == d->prof.big_offsets) {
        d->prof.big_launches++;
        d->prof.big_ms += ms;
    }
    return 0;
}

// What may still read the try list of the slot's previous launch comes first: the count pass over it is enqueued if it is
// still to come (count_flush), and `st`, where the next launch goes, waits for its end (count stream).
int slot_order_behind_count(adsb_decoder *d, ScanLaunch &s, hipStream_t st)
{
    if (d->pending.valid && d->pending.slot == &s && count_flush(d))
        return -1;
    if (s.count_pending) {
        HIP_TRY(d, hipStreamWaitEvent(st, s.ev_count, 0));
        s.count_pending = false;
    }
    return 0;
}

// Begin a launch on a slot, on stream `ls`: the event pair flips, the profile of the launch that used this copy last is
// settled, the launch is ordered behind the slot's previous one where that ran on the other stream, and it is given its tag
// and the slot's counters and loose list.
int slot_begin_launch(adsb_decoder *d, ScanSlot &s, hipStream_t ls, uint64_t offsets)
{
    s.ev_cur ^= 1;
    if (slot_settle_profile(d, s, s.ev_cur)) // two launches old: normally read long ago
        return -1;
    s.ev_offsets[s.ev_cur] = offsets;
    if (s.launch_stream && s.launch_stream != ls) // the slot's previous launch (its report kernel zeroes the counters) ran on the other stream
        HIP_TRY(d, hipStreamWaitEvent(ls, s.ev_ready[s.ev_cur ^ 1], 0));
    s.launch_stream = ls;
    s.args.gen = ++d->launch_gen * 0x9E3779B9u + 0x7F4A7C15u;
    // d_counters are zero here: cleared at creation, and the report kernel behind every scan leaves them so
    s.args.counters = s.d_counters;
    s.args.cands = s.cands;
    s.args.cand_cap = (uint32_t)std::min<size_t>(s.cand_cap, 0xFFFFFFFFu);
    s.args.profile = d->cfg.profile ? 1 : 0;
    s.args.report = s.hc();
    return 0;
}

int slot_launch(adsb_decoder *d, ScanSlot &s)
{
    const bool stats = d->cfg.collect_stats != 0;
    const int slot_index = (int)(&s - d->slots);
    hipStream_t ls = (d->alt_next && d->stream2 && (slot_index & 1)) ? d->stream2.st : d->stream.st;
    if (slot_begin_launch(d, s, ls, s.args.g_end - s.args.g_begin))
        return -1;
    s.ntiles = adsb::tile_count(s.args.g_end - s.args.g_begin, s.args.big_tiles, s.args.passes);
    // A stream's statistics run keeps the try words on the device (counted there after
    // resolution); a per-shard scan hands the list back, sorted, so it needs the list
    // complete on the host: collect after completion.
    s.tries_on_device = stats && !d->sink.cands;
    s.streaming = !d->no_streaming && (!stats || s.tries_on_device);
    if (s.streaming) {
        // a line per tile (marker + padding) + two granules per record (sized like the loose list)
        const size_t want_granules = 2 * s.cand_cap + 4 * (size_t)s.ntiles + 64;
        if (want_granules > s.hand_cap) {
            s.hand_cap = 0;
            HIP_TRY(d, s.hand.reserve(want_granules * adsb::kGranuleWords));
            s.hand_cap = want_granules;
        }
        s.args.hand = s.hand;
        s.args.hand_cap = (uint32_t)std::min<size_t>(s.hand_cap, 0xFFFFFFFFu);
    } else {
        s.args.hand = nullptr;
        s.args.hand_cap = 0;
    }
    if (slot_order_behind_count(d, s, ls))
        return -1;
    // debug_try_cap (tests of the relaunch path) wants every try on the launch-wide list
    s.try_regions = s.tries_on_device && d->dbg.try_cap <= 0;
    if (s.try_regions && slot_reserve_device_tries(d, s, s.d_try_cap, s.ntiles))
        return -1;
    s.args.tries = s.tries_on_device ? s.d_tries : s.tries;
    s.args.try_cap = (uint32_t)std::min<size_t>(s.tries_on_device ? s.d_try_cap : s.tries.cap, 0xFFFFFFFFu);
    s.args.try_counts = s.try_regions ? s.d_try_counts : nullptr;
    s.args.try_list_first = s.try_regions ? (uint32_t)(s.d_try_tiles * adsb::kTryRegion) : 0u;
    if (s.epoch_base) {
        // the kernel sees a fresh stream whose sample 0 is input sample w * 2^32: r mod 7, the run boundaries and the typed-load
        // alignment are the epoch's (P is a multiple of 4 pairs); pairs of the epoch before read as silence, and no offset of
        // this launch reads them (the first launch of an epoch starts at r = 28)
        adsb::ScanArgs ka = s.args;
        const int64_t P = (int64_t)s.epoch_base;
        ka.g_begin -= s.epoch_base;
        ka.g_end -= s.epoch_base;
        ka.pbuf0 -= P;
        ka.p_lo = std::max<int64_t>(ka.p_lo - P, 0);
        ka.p_hi -= P;
        HIP_TRY(d, adsb::launch_scan(ka, stats, ls));
    } else if (d->kind == adsb::kKindIq && !d->sink.cands) { // (a stateless shard scan on a handle that holds an IQ stream is a real one)
        HIP_TRY(d, adsb::launch_scan_iq(s.args, stats, ls));
    } else if (d->kind == adsb::kKindIq8 && !d->sink.cands) {
        HIP_TRY(d, adsb::launch_scan_iq8(s.args, stats, ls));
    } else if (d->kind == adsb::kKindPower && !d->sink.cands) {
        HIP_TRY(d, adsb::launch_scan_power(s.args, stats, ls));
    } else {
        HIP_TRY(d, adsb::launch_scan(s.args, stats, ls));
    }
    HIP_TRY(d, hipEventRecord(s.ev_ready[s.ev_cur], ls));
    if (stats && count_flush(d)) // the previous pass's calls are made now, while this scan runs
        return -1;
    for (ScanSlot &o : d->slots) // kernel times of earlier launches: read now, behind this launch
        for (int pair = 0; pair < 2; pair++)
            if (!(&o == &s && pair == s.ev_cur) && slot_settle_profile(d, o, pair))
                return -1;
    s.busy = true;
    return 0;
}

// Device-side visited-try count of a statistics run (scan_kernel.h TryCountArgs):
// decides every try below the resolver's position against the frames it accepted
// since the previous pass (plus the last one before, whose span may reach further),
// adds three counters to the statistics and carries the undecided tries.
// Everything here goes to the decoder's COUNT stream: the upload of the accepted frames and the count kernel
// (~40 us of device time together) run beside the next scan instead of in front of it.  Nothing on the scan
// stream depends on them except the reuse of the slot's try list, four launches later (ev_count); in the other
// direction the count stream waits for the end of the scan that wrote the list (count_flush).
// Enqueue the prepared count pass, if any (and the clearing an adsb_reset has queued behind it).
int count_flush(adsb_decoder *d)
{
    auto &p = d->pending;
    hipStream_t cs = d->count_stream;
    if (p.valid) {
        p.valid = false;
        if (p.nf) {
            HIP_TRY(d, hipMemcpyAsync(d->d_frames, p.src, p.nf * sizeof(adsb::TryFrame), hipMemcpyHostToDevice, cs));
            HIP_TRY(d, hipEventRecord(d->ev_frames[p.b], cs));
            d->frames_pending[p.b] = true;
        }
        // The host may have taken the launch's last tile before the scan kernel has ended (slot_collect does not
        // wait for the launch counters when no tile needed them): the try words become visible to other kernels
        // with the kernel's end, so the count stream waits for it.
        if (p.after)
            HIP_TRY(d, hipStreamWaitEvent(cs, p.after, 0));
        HIP_TRY(d, adsb::launch_count_tries(p.a, cs)); // enqueued and forgotten: read_tries() collects
        if (p.slot) {
            HIP_TRY(d, hipEventRecord(p.slot->ev_count, cs));
            p.slot->count_pending = true;
        }
    }
    if (p.clear_after) {
        p.clear_after = false;
        HIP_TRY(d, hipMemsetAsync(d->d_try_acc, 0, kTryStateBytes, cs));
    }
    return 0;
}

// `slot` is the launch whose tries are counted (null: none, the pass only decides what was carried), `tries` its try words --
// the regions first where the launch used them (`try_counts`), then the launch-wide list of n_tries words.
int count_tries_pass(adsb_decoder *d, ScanLaunch *slot, const uint32_t *tries, const uint32_t *try_counts, uint32_t n_tries,
                     uint64_t g_base, bool final)
{
    hipStream_t cs = d->count_stream;
    if (count_flush(d)) // one pass pending at a time, in order
        return -1;
    const bool regions = slot && slot->try_regions;
    static_assert(sizeof(adsb::Resolver::LogEntry) == sizeof(adsb::TryFrame), "the resolver logs TryFrame records in place");
    auto &over = d->res.accepted_log(); // entries that did not fit the pinned buffer (normally none)
    const size_t n_ext = d->res.logged_ext(), n_log = n_ext + over.size();
    const size_t nf = n_log + (d->have_prev_frame ? 1 : 0);
    int b = d->log_buf;
    const bool had_prev = d->have_prev_frame;
    const uint64_t prev_g = d->prev_frame_g;
    const uint32_t prev_span = d->prev_frame_span;
    if (n_log) { // the last accepted frame: its span may cover tries of the next pass
        d->have_prev_frame = true;
        if (!over.empty()) {
            d->prev_frame_g = over.back().first;
            d->prev_frame_span = over.back().second;
        } else {
            d->prev_frame_g = d->h_frames[b][n_ext].g; // entries sit at [1 .. n_ext]
            d->prev_frame_span = d->h_frames[b][n_ext].span;
        }
    }
    if (n_tries == 0 && !regions && !d->carry_maybe) {
        d->res.log_clear();
        return 0;
    }
    if (!over.empty() || nf > d->frames_cap) { // rare: grow the frame arrays (passes in flight use them: drain the stream first)
        WAIT_STREAM(d, cs, "the try-count stream");
        const size_t cap = std::max<size_t>(nf + nf / 4 + 1, 2 * d->frames_cap);
        adsb::Buf<adsb::TryFrame, adsb::Mem::Pinned> nh[adsb_decoder::kFrameBufs]; // (a failure below frees what is in them)
        for (auto &h : nh)
            HIP_TRY(d, h.reserve(cap));
        if (n_ext)
            std::memcpy(nh[b] + 1, d->h_frames[b] + 1, n_ext * sizeof(adsb::TryFrame));
        size_t k = 1 + n_ext;
        for (const auto &f : over)
            nh[b][k++] = adsb::TryFrame{f.first, f.second, 0};
        for (int i = 0; i < adsb_decoder::kFrameBufs; i++) {
            d->h_frames[i] = std::move(nh[i]);
            d->frames_pending[i] = false;
        }
        HIP_TRY(d, d->d_frames.reserve(cap));
        d->frames_cap = cap;
    }
    const adsb::TryFrame *src = d->h_frames[b] + 1;
    if (had_prev) {
        d->h_frames[b][0] = adsb::TryFrame{prev_g, prev_span, 0};
        src = d->h_frames[b];
    }
    {   // the resolver goes on logging into the buffer of the pass before last
        const int nb = (b + 1) % adsb_decoder::kFrameBufs;
        if (d->frames_pending[nb]) {
            WAIT_EVENT(d, d->ev_frames[nb], "the upload of the accepted frames");
            d->frames_pending[nb] = false;
        }
        d->log_buf = nb;
        d->res.log_into(reinterpret_cast<adsb::Resolver::LogEntry *>(d->h_frames[nb] + 1), d->frames_cap - 1);
    }
    const int c_in = d->carry_n_cur, c_out = (c_in + 1) % 3, c_next = (c_in + 2) % 3;
    adsb::TryCountArgs a{};
    a.tries = slot ? tries + slot->args.try_list_first : nullptr;
    a.n_tries = n_tries;
    a.regions = regions ? tries : nullptr;
    a.region_counts = regions ? try_counts : nullptr;
    a.n_tiles = regions ? slot->ntiles : 0;
    a.passes = slot ? slot->args.passes : 0;
    a.big_tiles = slot ? slot->args.big_tiles : 0;
    a.g_base = g_base;
    a.carry_in = d->d_carry[d->carry_cur];
    a.n_carry = d->d_carry_n + c_in;
    a.frames = d->d_frames;
    a.n_frames = (uint32_t)nf;
    a.hi = d->res.base(); // every offset below has been visited or jumped over
    a.final = final ? 1 : 0;
    a.carry_out = d->d_carry[d->carry_cur ^ 1];
    a.carry_cap = kCarryCap;
    a.n_carry_out = d->d_carry_n + c_out; // zero: cleared at creation / reset, or by the pass before last
    a.n_carry_next = d->d_carry_n + c_next;
    a.acc = d->d_try_acc;
    d->pending.valid = true;
    d->pending.a = a;
    d->pending.nf = nf;
    d->pending.b = b;
    d->pending.src = src;
    d->pending.slot = (slot && (n_tries || regions)) ? slot : nullptr;
    d->pending.after = d->pending.slot ? slot->ev_ready[slot->ev_cur] : nullptr;
    d->prof.tries += n_tries;
    d->carry_cur ^= 1;
    d->carry_n_cur = c_out;
    d->carry_maybe = !final;
    d->tries_unread = true;
    d->acc_dirty = true;
    return 0;
}

// The statistics are asked for: wait for the count passes and take the device's totals.
int read_tries(adsb_decoder *d)
{
    if (!d->tries_unread)
        return 0;
    if (count_flush(d))
        return -1;
    unsigned long long acc[4];
    HIP_TRY(d, hipMemcpyAsync(acc, d->d_try_acc, sizeof acc, hipMemcpyDeviceToHost, d->count_stream));
    WAIT_STREAM(d, d->count_stream, "the try-count stream");
    d->tries_unread = false;
    if (acc[3])
        return d->fail("undecided tries exceeded the carry buffer (%u entries)", kCarryCap);
    d->res.set_tries(acc[0], acc[1], acc[2]);
    return 0;
}

// What a seam launch over the offsets [g_begin, g_end) of the wrap at P is given: the buffer, the handle's settings and tables.
static adsb::SeamArgs seam_args(const adsb_decoder *d, const uint16_t *buf, uint64_t buf_first, uint64_t buf_n, uint64_t P, uint64_t g_begin,
                                uint64_t g_end)
{
    adsb::SeamArgs a{};
    a.x = reinterpret_cast<const uint32_t *>(buf);
    a.pbuf0 = (int64_t)(buf_first / 2);
    a.p_lo = a.pbuf0;
    a.p_hi = a.pbuf0 + (int64_t)(buf_n / 2);
    a.boundary = P;
    a.g_begin = g_begin;
    a.g_end = g_end;
    a.df18 = d->cfg.df18 ? 1 : 0;
    a.synd = d->d_synd;
    a.fix_tab = d->cfg.fix_1bit ? d->d_fix : nullptr;
    a.fix_mul = d->fix_mul;
    a.want_tries = d->cfg.collect_stats ? 1 : 0;
    a.out = d->seam_out;
    return a;
}

// Offsets [g_begin, g_end) among the seam offsets of the wrap at power sample P (seam_kernel.h): one small launch, waited for.
// Every launch before it is collected first, so its records reach the sink in offset order between those of the launches on
// either side, and its tries are counted by a pass of their own between theirs.  Once per 2^32 samples: the wait costs
// nothing that matters.
static int seam_scan(adsb_decoder *d, const uint16_t *buf, uint64_t buf_first, uint64_t buf_n, uint64_t P, uint64_t g_begin, uint64_t g_end)
{
    const bool stats = d->cfg.collect_stats != 0;
    if (!d->seam_out)
        return d->fail("internal: seam scan on a handle without adsb_set_long_stream");
    const bool ff = d->final_follows;
    d->final_follows = false; // (the launches in front are not the stream's last)
    const int rc = scan_drain(d);
    d->final_follows = ff;
    if (rc)
        return -1;
    ScanLaunch &s = d->seam_slot;
    if (slot_order_behind_count(d, s, d->stream)) // (statistics runs: the count pass over the previous seam launch's tries reads seam_out)
        return -1;
    const adsb::SeamArgs a = seam_args(d, buf, buf_first, buf_n, P, g_begin, g_end);
    HIP_TRY(d, adsb::launch_seam(a, d->stream));
    HIP_TRY(d, hipEventRecord(s.ev_ready[0], d->stream));
    WAIT_EVENT(d, s.ev_ready[0], "a seam launch");
    const size_t nc = d->seam_out[0], nt = d->seam_out[1];
    if (nc > (size_t)adsb::kSeamMaxOffsets || nt > (size_t)adsb::kSeamMaxOffsets)
        return d->fail("internal: a seam launch reported %zu records and %zu tries for %llu offsets", nc, nt, (unsigned long long)(g_end - g_begin));
    s.args = adsb::ScanArgs{};
    s.args.g_begin = g_begin; // the base of the records' and the try words' relative offsets
    s.args.g_end = g_end;
    s.ev_cur = 0;
    s.try_regions = false;
    const uint32_t *recs = d->seam_out + adsb::kSeamOutHeader;
    sort_order(d, recs, nc);
    const bool host_tries = stats && d->sink.cands;
    uint32_t *tries = d->seam_out + adsb::kSeamOutHeader + (size_t)adsb::kCandWords * adsb::kSeamMaxOffsets;
    if (host_tries && nt)
        sort_tries(d, tries, nt);
    deliver(d, s, recs, d->order.data(), nc, adsb::kCandWords, 0, tries, host_tries ? nt : 0, g_end);
    if (stats && !host_tries && nt) {
        if (count_tries_pass(d, &s, tries, nullptr, (uint32_t)nt, g_begin, false)) // (pinned host memory: the count kernel reads it where it lies)
            return -1;
    }
    d->seam_offsets += g_end - g_begin;
    d->prof.launches++;
    d->prof.offsets += g_end - g_begin;
    return 0;
}

// What every scan launch of the handle is given, whatever it scans: the settings of cfg, the tables, and the test knobs that
// shrink a tile's queues.
void fill_scan_args(const adsb_decoder *d, ScanArgs &a)
{
    a.df18 = d->cfg.df18 ? 1 : 0;
    a.synd = d->d_synd;
    a.queue_cap = (d->dbg.queue_cap >= 256 && d->dbg.queue_cap <= adsb::kQueueCap) ? d->dbg.queue_cap : adsb::kQueueCap;
    a.all_candidates = d->cfg.all_candidates ? 1 : 0;
    a.clist_cap = (d->dbg.clist_cap >= 1 && d->dbg.clist_cap <= adsb::kClistCap) ? d->dbg.clist_cap : adsb::kClistCap;
    a.fix_tab = d->cfg.fix_1bit ? d->d_fix.p : nullptr;
    a.fix_mul = d->fix_mul;
}

// Records and try words a launch of n_offsets offsets is given room for: far more than noise produces (a launch that needs
// more is repeated with exact sizes).  The test knobs start from buffers that are too small, so that the relaunch path runs;
// they bite on a slot whose buffers are still smaller than the knob only -- a fresh handle: slot_reserve never shrinks.
void scan_record_room(const adsb_decoder *d, uint64_t n_offsets, size_t *cand_want, size_t *try_want)
{
    *cand_want = d->dbg.cand_cap > 0 ? (size_t)d->dbg.cand_cap : (size_t)(n_offsets / 128 + 32768);
    *try_want = d->dbg.try_cap > 0 ? (size_t)d->dbg.try_cap : (size_t)(n_offsets / 32 + 65536);
}

// Submit offsets [g_begin, g_end) of a device buffer holding stream samples
// [buf_first, buf_first + buf_n) (buf_first % 8 == 0, buf 16-byte aligned) as a
// pipeline of chunked launches: while the device scans chunk k+1 the host sorts
// and resolves chunk k.  Records reach the sink in ascending g.
int scan_submit(adsb_decoder *d, const uint16_t *buf, uint64_t buf_first, uint64_t buf_n, uint64_t g_begin,
                uint64_t g_end)
{
    const bool stats = d->cfg.collect_stats != 0;
    while (g_begin < g_end) {
        uint64_t g_limit = g_end, epoch_base = 0;
        if (d->long_stream) {
            // A launch lies in ONE epoch.  The offsets [P - 1196, P + 28) around a wrap at P read a power sample that follows
            // neither epoch's formula (P - 1 .. P + 5): they go through the seam kernel, in their turn.
            const uint64_t P = round_down(g_begin, adsb::kEpoch), Pn = P + adsb::kEpoch;
            const uint64_t wrap = (P && g_begin < adsb::seam_end(P)) ? P : g_begin >= adsb::seam_first(Pn) ? Pn : 0;
            if (wrap) {
                const uint64_t g_stop = std::min(g_end, adsb::seam_end(wrap));
                if (seam_scan(d, buf, buf_first, buf_n, wrap, g_begin, g_stop))
                    return -1;
                g_begin = g_stop;
                continue;
            }
            g_limit = std::min(g_end, adsb::seam_first(Pn));
            epoch_base = P;
            if ((g_begin - P) % 28 != 0)
                return d->fail("internal: a scan launch at offset %llu does not start on a run boundary of its epoch", (unsigned long long)g_begin);
        }
        // streamed launches: everything but a per-shard scan that hands the try list back
        const uint64_t g_stop = std::min(g_limit, g_begin + chunk_offsets(!d->no_streaming && !(stats && d->sink.cands)));
        const uint64_t n_off = g_stop - g_begin;
        if (d->slot_count == kSlots && slot_collect(d))
            return -1;
        ScanSlot &s = d->slots[(d->slot_head + d->slot_count) % kSlots];
        const bool host_tries = stats && d->sink.cands; // per-shard scans return the try list
        size_t cand_want, try_want;
        scan_record_room(d, n_off, &cand_want, &try_want);
        if (slot_reserve(d, s, std::max<size_t>(s.cand_cap, cand_want),
                         host_tries ? std::max<size_t>(s.tries.cap, try_want) : s.tries.cap))
            return -1;
        if (stats && !host_tries && slot_reserve_device_tries(d, s, std::max<size_t>(s.d_try_cap, try_want), s.d_try_tiles))
            return -1;
        adsb::ScanArgs &a = s.args;
        a = adsb::ScanArgs{};
        a.x = reinterpret_cast<const uint32_t *>(buf);
        a.pbuf0 = (int64_t)(buf_first / 2);
        a.p_lo = a.pbuf0; // stream start: pairs below 0 read as silence (air.c:33)
        a.p_hi = a.pbuf0 + (int64_t)(buf_n / 2);
        if (d->flush) // the silent twin ends at the stream's last whole pair of power samples: a trailing partial quad (an odd IQ
                      // or power sample) belongs to nothing, and only the stream's last launch could have read it
            a.p_hi = std::min<int64_t>(a.p_hi, (int64_t)power_samples_produced(d->n_samples));
        a.g_begin = g_begin;
        a.g_end = g_stop;
        fill_scan_args(d, a);
        // (choose_passes's table was measured with the real kernel; IQ and int8 IQ launches use it as it is: nobody has measured theirs)
        a.passes = (d->dbg.passes >= 2 && d->dbg.passes <= adsb::kMaxPasses) ? d->dbg.passes
                                                                                         : adsb::choose_passes(n_off, d->n_cus, last_launch_was_dense(d));
        a.big_tiles = adsb::choose_big_tiles(n_off, a.passes, d->n_cus, d->dbg.big_tiles);
        s.epoch_base = epoch_base;
        if (slot_launch(d, s))
            return -1;
        s.piece = d->piece;
        d->slot_count++;
        g_begin = g_stop;
    }
    return 0;
}

// Where the kept tail of the staging buffer starts: at or below `want` (a multiple of 8 samples), lowered by up
// to 56 samples so that the tail's END -- where the next push is appended -- falls on a 128-byte line whenever
// the stream position allows it (n_samples % 8 == 0): pieces of adsb_push_async that start on a line run on
// alternating copy streams without waiting for each other (push_copy).
static uint64_t line_aligned_keep(uint64_t want, uint64_t n_samples, uint64_t floor_first)
{
    if (n_samples % 8 != 0 || want > n_samples)
        return want;
    const uint64_t extra = (64 - (n_samples - want) % 64) % 64; // samples; a multiple of 8
    return want >= floor_first + extra ? want - extra : want;
}

// Scan what the staged samples allow, resolve, and keep only the unscanned tail.
// in_flight (adsb_push_async): the launches submitted here are left running; only those
// of earlier pieces are collected.
int process_stage(adsb_decoder *d, bool final, bool in_flight)
{
    const uint64_t m_real = power_samples_produced(d->n_samples);
    const uint64_t g_end = scannable_end(d, d->n_samples, final);
    bool launched = false;
    if (g_end > d->g_scanned) {
        if (scan_submit(d, d->stage[d->cur], d->stage_first, d->stage_fill, d->g_scanned, g_end))
            return -1;
        d->g_scanned = g_end;
        launched = true;
    }
    if (in_flight) {
        while (d->slot_count && d->slots[d->slot_head].piece < d->piece)
            if (slot_collect(d))
                return -1;
    } else {
        if (scan_drain(d)) // frames become drainable within the call that supplied their samples
            return -1;
        if (launched) // its tiles have all been taken: the scan, and with it every copy queued in front of it, is over
            d->copy_unconfirmed = false;
    }
    // At EOF a trailing partial quad still makes the reference produce two (garbage)
    // power samples (air.c:59 loop bound); they can never be read by a visited
    // offset but they count for the `aidx >= APBUFFSZ` test.
    // (An IQ or power stream has no quads: its power samples enter two at a time and a trailing odd one is never seen.)
    const uint64_t m_ref = final && !adsb::kind_in_twos(d->kind) ? 2 * ((d->n_samples + 3) / 4) : m_real;
    if (!in_flight) { // (in flight: the records below g_scanned are not all in yet; slot_collect advanced as far as they are)
        const adsb::StreamEnd e = adsb::stream_end(final && d->flush && !d->shard_on, m_real, m_ref, d->g_scanned);
        d->res.advance(e.power_samples, e.g_complete);
    }
    if (final)
        return 0;

    // Keep samples from pair (g_scanned - 8) on; that index is a multiple of 8 samples.  The
    // scanned part is only dropped (the tail moved to the other buffer) once the buffer is
    // half full: until then the next push is appended behind what is there and the next scan
    // reads [tail | new] where it lies -- small pushes (the reference's 1 Mi-sample calls)
    // then cost no device-to-device copy at all.
    const uint64_t keep_first = line_aligned_keep(d->g_scanned >= 8 ? 2 * (d->g_scanned - 8) : 0, d->n_samples, d->stage_first);
    if (keep_first > d->stage_first && d->stage_fill > (d->stage_cap - kStageSlack) / 2) {
        const uint64_t skip = keep_first - d->stage_first;
        const uint64_t left = d->stage_fill > skip ? d->stage_fill - skip : 0;
        if (left) {
            // The next asynchronous piece is copied right behind this tail by a copy engine on another stream,
            // and the two ranges meet inside a cache line (when `left` is not line-aligned): unordered, the tail
            // copy's write-back of that line and the engine's write to it race, and the loser's bytes are lost
            // (observed: one frame straddling the seam missing in 5-35 % of the runs with a 64 Ki staging buffer,
            // which compacts at every piece; tools/async_race.py).  So every later copy waits for the tail copy.
            // The tail copy itself needs this piece's copy and nothing else -- the buffer it writes was last read
            // by launches that have been collected, and it only reads the current one -- so in asynchronous mode
            // it follows that copy on ITS stream instead of queueing behind this piece's scan: the bubble per
            // compaction is the tail copy (a few KB), not a scan.
            const bool aside = in_flight && d->dbg_async != 4 && d->dbg_async != 2;
            hipStream_t ts = aside ? d->copy_stream[d->piece % adsb_decoder::kCopyStreams].st : d->stream.st;
            // The tail also holds the end of the PREVIOUS piece whenever this piece is shorter than the tail
            // (~2.5 K samples), and that piece was copied on the other copy stream: order behind it too (an event
            // that has already completed costs nothing).
            if (aside && d->piece > 1)
                HIP_TRY(d, hipStreamWaitEvent(ts, d->ev_copy[(d->piece - 1) % adsb_decoder::kCopyStreams], 0));
            // (an int8 IQ stream's units are bytes, an even number of them: left / 2 16-bit words from byte `skip` on)
            HIP_TRY(d, adsb::launch_copy_samples(d->stage[d->cur ^ 1], stage_at(d, d->cur, skip), (left * adsb::kind_unit_bytes(d->kind) + 1) / 2, ts)); // (the library's own kernel:
            //                                the runtime's first device-to-device copy of a process costs 7 ms, scan_kernel.hip)
            // Behind EVERY tail copy, the one of a synchronous push on the scan stream included: a following
            // adsb_push_async copies right behind this tail on a copy stream that nothing else orders against it.
            if (d->dbg_async != 4) {
                HIP_TRY(d, hipEventRecord(d->ev_tail, ts));
                if (ts != d->stream)
                    HIP_TRY(d, hipStreamWaitEvent(d->stream, d->ev_tail, 0));
                for (hipStream_t cs : d->copy_stream)
                    if (cs != ts)
                        HIP_TRY(d, hipStreamWaitEvent(cs, d->ev_tail, 0));
            }
        }
        d->cur ^= 1;
        d->stage_first = keep_first;
        d->stage_fill = left;
    }
    return 0;
}

// async (adsb_push_async): the copy of a piece goes to the copy stream and the scan stream
// waits for it by event, so that the copy engine moves piece k+1 while piece k is scanned;
// the launches of a piece are collected while the NEXT piece is on its way.  Why no other
// synchronisation is needed: piece k is copied behind the unscanned tail of the staging
// buffer that becomes current after piece k-1's tail copy, [left, left + take) -- a region
// that the tail copy (it writes [0, left)) does not touch, that scan k-1 does not read (it
// reads the other buffer, or this one below `left`), and whose previous reader, scan k-2,
// was collected while piece k-1 was pushed.
// packed (adsb_push_packed*): src holds n / 8 groups of packed 12-bit samples (n % 8 == 0, stage_fill % 8 == 0).  The
// copy lands them in land[] and the unpack kernel writes the samples where the copy would have, on the copy's stream,
// before the copy's event: to everything that orders against the copies it is part of the copy.
// conv (adsb_push_as, adsb_push_async_as: kFmtInt16Real / kFmtFloat32Real): src holds n samples of that format; they land in
// land[] like packed ones and the conversion kernel stands where the unpack does.  Any n, any stage_fill.
static int push_copy(adsb_decoder *d, const void *src, size_t n, hipMemcpyKind kind, bool async = false, bool packed = false, int conv = 0)
{
    const size_t elem = adsb::convert_element_bytes(conv), unit = adsb::kind_unit_bytes(d->kind);
    const char *p = static_cast<const char *>(src);
    while (n) {
        uint64_t room = d->stage_cap - kStageSlack - d->stage_fill;
        if (packed)
            room = round_down(room, adsb::kPackedGroupSamples);
        if (room == 0)
            return d->fail("staging buffer exhausted (stage_samples too small)");
        const size_t take = (size_t)std::min<uint64_t>(room, n);
        const size_t bytes = packed ? take / adsb::kPackedGroupSamples * adsb::kPackedGroupBytes : conv ? take * elem : take * unit;
        // the piece to stage[cur] + stage_fill on `st`: as it is, or landed in `land` and unpacked or converted from there
        auto piece_to_stage = [&](uint8_t *land, hipStream_t st) -> int {
            HIP_TRY(d, hipMemcpyAsync(packed || conv ? (void *)land : (void *)stage_at(d, d->cur, d->stage_fill), p, bytes, kind, st));
            if (packed)
                HIP_TRY(d, adsb::launch_unpack12(stage_at(d, d->cur, d->stage_fill), land, take / adsb::kPackedGroupSamples, st));
            else if (conv)
                HIP_TRY(d, adsb::launch_convert(conv, stage_at(d, d->cur, d->stage_fill), land, take, d->d_fmt, st));
            return 0;
        };
        if (async) {
            d->piece++;
            const int cs = (int)(d->piece % adsb_decoder::kCopyStreams);
            hipStream_t cstream = d->dbg_async == 2 ? d->stream.st : d->copy_stream[cs].st;
            // Same rule as for the tail copy in process_stage: two writers that are not ordered never share a
            // cache line.  A piece that starts inside a 128-byte line (pushes of odd sizes) waits for the copy of
            // the piece before it, which ends in that line.
            if (d->piece > 1 && (d->stage_fill * unit) % 128 != 0 && d->dbg_async != 2)
                HIP_TRY(d, hipStreamWaitEvent(cstream, d->ev_copy[cs ^ 1], 0));
            if (piece_to_stage(d->land[cs], cstream))
                return -1;
            HIP_TRY(d, hipEventRecord(d->ev_copy[cs], cstream));
            if (d->dbg_async != 2)
                HIP_TRY(d, hipStreamWaitEvent(d->stream, d->ev_copy[cs], 0));
            if (d->dbg_async == 1)
                WAIT_STREAM(d, cstream, "a copy stream");
        } else {
            // (packed: land[0] -- an earlier asynchronous piece that used it is ordered in front by its event, and an earlier
            // synchronous push was complete when it returned)
            if (piece_to_stage(d->land[0], d->stream))
                return -1;
            d->copy_unconfirmed = true;
        }
        d->stage_fill += take;
        d->n_samples += take;
        if (conv) {
            d->fmt_converted += take;
            d->fmt_dirty = true;
        }
        p += bytes;
        n -= take;
        if (process_stage(d, false, async))
            return -1;
        if (async && d->piece > 1) {
            // adsb_push_async's contract: the buffer of the PREVIOUS piece is free when this call
            // returns.  Collecting that piece's scan implies it; a piece too small to launch a
            // scan leaves only its copy to wait for (already complete in every other case).
            WAIT_EVENT(d, d->ev_copy[(d->piece - 1) % adsb_decoder::kCopyStreams], "the host-to-device copy of the previous piece");
        }
    }
    return 0;
}

// The rules every packed push checks before it changes anything: whole groups, at stream position `at` (a multiple of 8).
static int packed_refusal(adsb_decoder *d, const char *what, size_t n, uint64_t at)
{
    if (n % adsb::kPackedGroupSamples != 0)
        return d->fail("%s: n = %zu is not a multiple of 8 (packed 12-bit input comes in whole 8-sample groups)", what, n);
    if (at % adsb::kPackedGroupSamples != 0)
        return d->fail("%s at stream position %llu: packed input must start at a multiple of 8 samples", what,
                       (unsigned long long)at);
    return 0;
}

// The converted formats (adsb_*_as; sample_format.h).  What a call needs before its first conversion: the two counters, and
// landing buffers of land_bytes each (0: none; a host push lands its samples there as a packed one does).  A buffer that has to
// grow is released first, so what may still read or write it -- an earlier piece's copy or unpack -- is waited for.
int format_prepare(adsb_decoder *d, const char *what, size_t land_bytes)
{
    if (!d->d_fmt) {
        if (d->d_fmt.reserve(2) != hipSuccess) {
            (void)hipGetLastError();
            return d->fail("%s: cannot allocate the format counters on the device", what);
        }
        HIP_TRY(d, hipMemsetAsync(d->d_fmt, 0, 2 * sizeof(unsigned long long), d->stream));
        WAIT_STREAM(d, d->stream, "the scan stream");
    }
    for (auto &l : d->land) {
        if (l.cap >= land_bytes)
            continue;
        for (hipStream_t cs : d->copy_stream)
            WAIT_STREAM(d, cs, "a copy stream");
        WAIT_STREAM(d, d->stream, "the scan stream");
        if (l.reserve(land_bytes) != hipSuccess) {
            (void)hipGetLastError();
            return d->fail("%s: cannot allocate a landing buffer of %zu bytes on the device", what, land_bytes);
        }
    }
    return 0;
}

// The two counters as the device has them once every conversion enqueued so far has ended.
int format_counters(adsb_decoder *d, unsigned long long out[2])
{
    out[0] = out[1] = 0;
    if (!d->d_fmt)
        return 0;
    HIP_TRY(d, hipSetDevice(d->device));
    for (hipStream_t cs : d->copy_stream)
        WAIT_STREAM(d, cs, "a copy stream");
    HIP_TRY(d, hipMemcpyAsync(out, d->d_fmt, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, d->stream));
    WAIT_STREAM(d, d->stream, "the scan stream");
    return 0;
}

// The stream's kind is fixed by its first push with samples; a push of another kind is refused, the handle as it was.
int kind_refusal(adsb_decoder *d, const char *what, int kind)
{
    static const char *const names[] = {"", "real", "IQ (fmt 0 / 2)", "power", "int8 IQ (fmt 8)"};
    if (adsb::kind_in_twos(kind) && d->long_stream)
        return d->fail("%s: a long-stream handle (adsb_set_long_stream) takes real samples only, not %s ones: the counter wrap it follows is "
                       "the FIR ring's (air.c:34) and %s stream has no ring", what, names[kind], kind == adsb::kKindPower ? "a power" : "an IQ");
    if (d->kind != adsb::kKindNone && d->kind != kind)
        return d->fail("%s: the stream holds %s samples (its first push fixed that) and %s samples cannot follow them: adsb_reset starts a "
                       "fresh stream", what, names[d->kind], names[kind]);
    return 0;
}

// adsb_push, adsb_push_async and their packed forms: samples in host memory (`packed`: whole groups of 12-bit samples).
// kind: kKindIq from the _iq calls, whose n counts 16-bit units (fmt 2) or float scalars (fmt 0): two per complex sample;
// kKindIq8 from the _iq calls with fmt 8, whose n counts BYTES: two per complex sample (kind_unit_bytes);
// kKindPower from the _power calls, whose n counts 16-bit units too: two per power sample.
static int push_host(adsb_decoder *d, const void *samples, size_t n, bool async, bool packed, const char *what, int conv = 0,
                     int kind = adsb::kKindReal)
{
    if (!d)
        return -1;
    if (d->finished)
        return d->fail("%s after adsb_finish", what);
    if (kind_refusal(d, what, kind) || (packed && packed_refusal(d, what, n, d->n_samples)) || stream_too_long(d, n))
        return -1;
    if (n == 0)
        return 0;
    if (!samples)
        return d->fail("%s: NULL samples", what);
    d->kind = kind;
    HIP_TRY(d, hipSetDevice(d->device));
    if (packed) { // the landing buffers, one per copy stream: a handle that never sees packed input has none
        const size_t bytes = d->stage_cap / adsb::kPackedGroupSamples * adsb::kPackedGroupBytes;
        for (auto &l : d->land)
            if (l.reserve(bytes) != hipSuccess) {
                (void)hipGetLastError();
                return d->fail("packed input: cannot allocate a landing buffer of %zu bytes on the device", bytes);
            }
    }
    if (conv && format_prepare(d, what, d->stage_cap * adsb::convert_element_bytes(conv)))
        return -1;
    if (async)
        return push_copy(d, samples, n, hipMemcpyHostToDevice, true, packed, conv);
    if (d->cfg.push_overlap) {
        // The caller's ONE buffer (fileInput's iqbuff, air.c:230-239; the callback's transfer, air.c:173-177) is
        // only borrowed until its bytes are on the device: return when the COPY (packed: copy + unpack) has completed and
        // leave the scan in flight -- the host is back in read() while the device scans, and this call has meanwhile collected
        // the frames of the previous one (frames arrive one call late, never reordered; adsb_finish / adsb_sync
        // deliver the rest).  That is adsb_push_async plus the wait for this piece's own copy.
        if (push_copy(d, samples, n, hipMemcpyHostToDevice, true, packed, conv))
            return -1;
        return wait_last_copy(d);
    }
    if (push_copy(d, samples, n, hipMemcpyHostToDevice, false, packed, conv))
        return -1;
    if (d->copy_unconfirmed) { // `samples` is only borrowed for the call: no scan behind the last copy has confirmed it
        WAIT_STREAM(d, d->stream, "the scan stream");
        d->copy_unconfirmed = false;
    }
    return 0;
}

// adsb_push_device, optionally followed by adsb_finish in the same pass (`final`):
// the last in-place scan then runs to the exact end of the stream and no tail has to
// be staged.
static int push_device_impl(adsb_decoder *d, const void *device_samples, size_t n, bool final, int kind = adsb::kKindReal)
{
    if (!d)
        return -1;
    if (d->finished)
        return d->fail("adsb_push_device after adsb_finish");
    if (final && d->shard_on)
        return d->fail("a shard stream ends with adsb_shard_end");
    if (kind_refusal(d, "adsb_push_device", kind) || stream_too_long(d, n))
        return -1;
    if (n && !device_samples)
        return d->fail("adsb_push_device: NULL samples");
    if (n)
        d->kind = kind;
    HIP_TRY(d, hipSetDevice(d->device));
    // p[0] is unit d->n_samples of the stream; a unit is 16 bits, or a byte of an int8 IQ stream (kind_unit_bytes)
    const uint16_t *p = static_cast<const uint16_t *>(device_samples);
    const size_t unit = adsb::kind_unit_bytes(kind);
    const bool aligned = (d->n_samples % 8 == 0) && ((uintptr_t)p % 16 == 0);
    if (!aligned || n < kInPlaceMinSamples) {
        if (n && push_copy(d, p, n, hipMemcpyDeviceToDevice))
            return -1;
        if (final)
            return adsb_finish(d);
        // the staging copy may still be queued when no scan was launched behind it (and
        // collected): the caller is free to reuse or free the buffer on return
        if (d->copy_unconfirmed) {
            WAIT_STREAM(d, d->stream, "the scan stream");
            d->copy_unconfirmed = false;
        }
        return 0;
    }

    // In-place scan.  First the seam: offsets whose window starts in earlier data.
    const uint64_t first = d->n_samples; // stream index of p[0]
    if (first != d->stage_first || d->stage_fill != 0) { // (not at the very start of a stream or of a shard: nothing earlier exists)
        if (push_copy(d, p, kSeamSamples, hipMemcpyDeviceToDevice))
            return -1;
    }
    // Bulk: every offset whose whole window lies inside this buffer.
    const uint64_t total = first + n;
    const uint64_t m_real = power_samples_produced(total);
    const uint64_t g_end = scannable_end(d, total, final);
    d->n_samples = total;
    if (final) {
        using clk = std::chrono::steady_clock;
        const bool dbg_on = tuning_env("ADSB_DEBUG_HOST") != nullptr;
        const auto t0 = clk::now();
        if (g_end > d->g_scanned) {
            d->alt_next = true; // in place: nothing on d->stream has to precede these launches
            const int rc_submit = scan_submit(d, p, first, n, d->g_scanned, g_end);
            d->alt_next = false;
            if (rc_submit)
                return -1;
            d->g_scanned = g_end;
        }
        const auto t1 = clk::now();
        d->final_follows = true;
        d->deferred_n = 0, d->deferred_slot = nullptr;
        const int rc = scan_drain(d);
        d->final_follows = false;
        if (rc)
            return -1;
        const auto t2 = clk::now();
        const adsb::StreamEnd e = adsb::stream_end(d->flush, m_real, adsb::kind_in_twos(d->kind) ? m_real : 2 * ((total + 3) / 4), d->g_scanned);
        d->res.advance(e.power_samples, e.g_complete); // EOF rule: see process_stage()
        if (d->cfg.collect_stats && count_tries_pass(d, d->deferred_slot, d->deferred_slot ? d->deferred_slot->d_tries.p : nullptr,
                                                        d->deferred_slot ? d->deferred_slot->d_try_counts.p : nullptr, d->deferred_n, d->deferred_base, true))
            return -1; // tries beyond the final position are never visited
        d->stage_fill = 0;
        d->finished = true;
        if (dbg_on) {
            auto us = [](clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); };
            fprintf(stderr, "push_device_final: submit %.1f us, drain %.1f us, finish %.1f us\n", us(t0, t1), us(t1, t2),
                    us(t2, clk::now()));
        }
        return 0;
    }
    // Tail first: what the next push (or adsb_finish) still needs goes to the staging
    // buffer.  Issued ahead of the scans so that it is finished, in stream order, by
    // the time the last scan is collected (the caller may free the buffer on return).
    const uint64_t g_after = std::max(g_end, d->g_scanned);
    const uint64_t keep_first = line_aligned_keep(std::max<uint64_t>(g_after >= 8 ? 2 * (g_after - 8) : 0, first), total, first);
    const uint64_t left = total - keep_first;
    if (left > d->stage_cap - kStageSlack)
        return d->fail("in-place tail (%llu samples) exceeds the staging buffer", (unsigned long long)left);
    d->cur ^= 1; // the seam scan above may still be reading the other buffer
    HIP_TRY(d, adsb::launch_copy_samples(d->stage[d->cur], reinterpret_cast<const uint16_t *>(static_cast<const char *>(device_samples) + (keep_first - first) * unit),
                                         (left * unit + 1) / 2, d->stream));
    d->stage_first = keep_first;
    d->stage_fill = left;
    if (g_end > d->g_scanned) {
        d->alt_next = true;
        const int rc_submit = scan_submit(d, p, first, n, d->g_scanned, g_end);
        d->alt_next = false;
        if (rc_submit)
            return -1;
        d->g_scanned = g_end;
    } else {
        WAIT_STREAM(d, d->stream, "the scan stream");
    }
    if (scan_drain(d))
        return -1;
    if (d->stream2) // the launches may all have gone to the second stream: the tail copy is not implied by their end
        WAIT_STREAM(d, d->stream, "the scan stream");
    d->res.advance(m_real, d->g_scanned);
    return 0;
}

// adsb_push_device_packed*: unpack into the handle's scratch (grown to 2 B x n on demand), then push that in place.
// The checks come first: a refused push leaves the handle as it was.
static int packed_device_refusal(adsb_decoder *d, const void *device_packed, size_t n, uint64_t at, const char *what)
{
    if (packed_refusal(d, what, n, at))
        return -1;
    if ((uintptr_t)device_packed % 4 != 0)
        return d->fail("%s: device pointer %p is not 4-byte aligned", what, device_packed);
    if (n && !device_packed)
        return d->fail("%s: NULL samples", what);
    return 0;
}

// What adsb_push_device_packed* and adsb_push_device_as and their kin do behind their refusals: unpack or convert into the handle's
// scratch (decoder_stage.hip; conv = 0: unpack), then push that in place -- its launches alternate onto the second scan stream,
// which waits for the scratch.
static int push_device_scratch(adsb_decoder *d, int conv, const void *p, size_t n, bool final, const char *what, int kind)
{
    if (n == 0)
        return final ? push_device_impl(d, nullptr, 0, true, kind) : 0;
    if (adsb::to_scratch(d, what, conv, p, n) || adsb::scratch_before_stream2(d))
        return -1;
    return push_device_impl(d, d->unpacked, n, final, kind);
}

static int push_device_packed_impl(adsb_decoder *d, const void *device_packed, size_t n, bool final, const char *what)
{
    if (d->finished)
        return d->fail("%s after adsb_finish", what);
    if (final && d->shard_on)
        return d->fail("a shard stream ends with adsb_shard_end");
    if (kind_refusal(d, what, adsb::kKindReal) || packed_device_refusal(d, device_packed, n, d->n_samples, what) || stream_too_long(d, n))
        return -1;
    return push_device_scratch(d, 0, device_packed, n, final, what, adsb::kKindReal);
}

// adsb_push_device_as and its kin: the checks first (a refused push leaves the handle as it was), at stream position `at`
static int device_as_refusal(adsb_decoder *d, const char *what, const void *p, size_t n, size_t elem)
{
    if ((uintptr_t)p % elem != 0)
        return d->fail("%s: device pointer %p is not %zu-byte aligned", what, p, elem);
    if (n && !p)
        return d->fail("%s: NULL samples", what);
    return 0;
}

// convert into the scratch of the packed device pushes (grown to 2 B x n on demand), then push that in place
// (kind: kKindIq from the _iq calls with fmt = kConvFloat32Iq, n counting float scalars)
static int push_device_as_impl(adsb_decoder *d, int fmt, const void *p, size_t n, bool final, const char *what, int kind = adsb::kKindReal)
{
    if (d->finished)
        return d->fail("%s after adsb_finish", what);
    if (final && d->shard_on)
        return d->fail("a shard stream ends with adsb_shard_end");
    if (kind_refusal(d, what, kind) || device_as_refusal(d, what, p, n, adsb::convert_element_bytes(fmt)) || stream_too_long(d, n))
        return -1;
    return push_device_scratch(d, fmt, p, n, final, what, kind);
}

// ---- complex samples (the _iq calls; include/adsbdec_amd.h) ----
// (what every _iq call checks first, and the stream kind a format makes: flavour.hpp iq_refusal, iq_kind)
static int push_host_iq(adsb_decoder *d, int fmt, const void *samples, size_t n, bool async, const char *what)
{
    if (!d)
        return -1;
    if (iq_refusal(d, what, fmt, samples, n, false, d->n_samples))
        return -1;
    return push_host(d, samples, 2 * n, async, false, what, fmt == 0 ? adsb::kConvFloat32Iq : 0, iq_kind(fmt));
}

// fmt 2 is scanned where it lies under the uint16 rule (16-byte aligned, at a multiple of 4 complex samples; else staged), and so
// is fmt 8 (scan_iq8_kernel.hip's lanes are then 8-byte aligned; its typed 4-byte loads ask for less);
// fmt 0 is converted into the scratch of the other converted device pushes first.
static int push_device_iq(adsb_decoder *d, int fmt, const void *p, size_t n, bool final, const char *what, bool checked = false)
{
    if (!d)
        return -1;
    if (!checked && iq_refusal(d, what, fmt, p, n, true, d->n_samples))
        return -1;
    if (d->finished)
        return d->fail("%s after adsb_finish", what);
    if (kind_refusal(d, what, iq_kind(fmt)))
        return -1;
    if (n == 0 && !final)
        return 0;
    if (fmt == 0)
        return push_device_as_impl(d, adsb::kConvFloat32Iq, p, 2 * n, final, what, adsb::kKindIq);
    return push_device_impl(d, p, 2 * n, final, iq_kind(fmt));
}

// ---- float32 power samples (the _power calls; include/adsbdec_amd.h) ----
// (what every _power call checks first: flavour.hpp power_refusal)
static int push_host_power(adsb_decoder *d, const float *samples, size_t n, bool async, const char *what)
{
    if (!d)
        return -1;
    if (power_refusal(d, what, samples, n, false, d->n_samples))
        return -1;
    return push_host(d, samples, 2 * n, async, false, what, 0, adsb::kKindPower);
}

// scanned where it lies under the uint16 rule (16-byte aligned, at a multiple of 4 power samples; else staged)
static int push_device_power(adsb_decoder *d, const void *p, size_t n, bool final, const char *what, bool checked = false)
{
    if (!d)
        return -1;
    if (!checked && power_refusal(d, what, p, n, true, d->n_samples))
        return -1;
    if (d->finished)
        return d->fail("%s after adsb_finish", what);
    if (kind_refusal(d, what, adsb::kKindPower))
        return -1;
    if (n == 0 && !final)
        return 0;
    return push_device_impl(d, p, 2 * n, final, adsb::kKindPower);
}

} // namespace adsb

extern "C" {

int adsb_push_power(adsb_decoder *d, const float *samples, size_t n)
{
    return push_host_power(d, samples, n, false, "adsb_push_power");
}

int adsb_push_power_async(adsb_decoder *d, const float *samples, size_t n)
{
    return push_host_power(d, samples, n, true, "adsb_push_power_async");
}

int adsb_push_device_power(adsb_decoder *d, const void *device_samples, size_t n)
{
    return push_device_power(d, device_samples, n, false, "adsb_push_device_power");
}

int adsb_push_device_power_final(adsb_decoder *d, const void *device_samples, size_t n)
{
    return push_device_power(d, device_samples, n, true, "adsb_push_device_power_final");
}

long adsb_decode_device_power(adsb_decoder *d, const void *device_samples, size_t n, const adsb_frame **frames)
{
    const char *what = "adsb_decode_device_power";
    if (!d || !frames)
        return -1;
    // refused before the reset, at the position the reset will set: a refused call leaves the handle as it was
    if (power_refusal(d, what, device_samples, n, true, 0) || (d->long_stream && kind_refusal(d, what, adsb::kKindPower)))
        return -1;
    if (adsb_reset(d) != 0 || push_device_power(d, device_samples, n, true, what, true) != 0)
        return -1;
    return (long)d->res.take(frames);
}

size_t adsb_iq_bytes(int fmt, size_t n)
{
    return adsb::iq_sample_bytes(fmt) * n;
}

int adsb_push_iq(adsb_decoder *d, int fmt, const void *samples, size_t n)
{
    return push_host_iq(d, fmt, samples, n, false, "adsb_push_iq");
}

int adsb_push_iq_async(adsb_decoder *d, int fmt, const void *samples, size_t n)
{
    return push_host_iq(d, fmt, samples, n, true, "adsb_push_iq_async");
}

int adsb_push_device_iq(adsb_decoder *d, int fmt, const void *device_samples, size_t n)
{
    return push_device_iq(d, fmt, device_samples, n, false, "adsb_push_device_iq");
}

int adsb_push_device_iq_final(adsb_decoder *d, int fmt, const void *device_samples, size_t n)
{
    return push_device_iq(d, fmt, device_samples, n, true, "adsb_push_device_iq_final");
}

long adsb_decode_device_iq(adsb_decoder *d, int fmt, const void *device_samples, size_t n, const adsb_frame **frames)
{
    const char *what = "adsb_decode_device_iq";
    if (!d || !frames)
        return -1;
    // refused before the reset, at the position the reset will set: a refused call leaves the handle as it was
    if (iq_refusal(d, what, fmt, device_samples, n, true, 0) || (d->long_stream && kind_refusal(d, what, iq_kind(fmt))))
        return -1;
    if (adsb_reset(d) != 0 || push_device_iq(d, fmt, device_samples, n, true, what, true) != 0)
        return -1;
    return (long)d->res.take(frames);
}

int adsb_convert_iq_float32(void *dst_i16, const void *src, size_t n_scalars, uint64_t *device_counters2, void *stream)
{
    char why[200] = "";
    if (n_scalars && (!dst_i16 || !src))
        snprintf(why, sizeof why, "adsb_convert_iq_float32: NULL buffer");
    else if ((uintptr_t)dst_i16 % 2 != 0 || (uintptr_t)src % 4 != 0 || (uintptr_t)device_counters2 % 8 != 0)
        snprintf(why, sizeof why, "adsb_convert_iq_float32: dst must be 2-byte, src 4-byte and the counters 8-byte aligned (%p, %p, %p)", dst_i16, src,
                 (void *)device_counters2);
    else if (n_scalars) {
        const hipError_t e = adsb::launch_convert(adsb::kConvFloat32Iq, static_cast<uint16_t *>(dst_i16), src, n_scalars,
                                                  reinterpret_cast<unsigned long long *>(device_counters2), static_cast<hipStream_t>(stream));
        if (e != hipSuccess)
            snprintf(why, sizeof why, "adsb_convert_iq_float32: launch failed: %s", hipGetErrorString(e));
    }
    if (!why[0])
        return 0;
    set_create_error(why);
    return -1;
}

int adsb_push(adsb_decoder *d, const uint16_t *samples, size_t n)
{
    return push_host(d, samples, n, false, false, "adsb_push");
}

int adsb_push_async(adsb_decoder *d, const uint16_t *samples, size_t n)
{
    return push_host(d, samples, n, true, false, "adsb_push_async");
}

int adsb_push_packed(adsb_decoder *d, const void *packed, size_t n)
{
    return push_host(d, packed, n, false, true, "adsb_push_packed");
}

int adsb_push_packed_async(adsb_decoder *d, const void *packed, size_t n)
{
    return push_host(d, packed, n, true, true, "adsb_push_packed_async");
}

int adsb_sync(adsb_decoder *d)
{
    if (!d)
        return -1;
    HIP_TRY(d, hipSetDevice(d->device));
    if (scan_drain(d))
        return -1;
    if (!d->finished)
        d->res.advance(power_samples_produced(d->n_samples), d->g_scanned);
    for (hipStream_t cs : d->copy_stream)
        WAIT_STREAM(d, cs, "a copy stream");
    WAIT_STREAM(d, d->stream, "the scan stream"); // tail copies: every borrowed buffer is free
    if (d->stream2)
        WAIT_STREAM(d, d->stream2, "the second scan stream");
    return 0;
}


int adsb_push_device(adsb_decoder *d, const void *device_samples, size_t n)
{
    if (n == 0 && d && !d->finished)
        return 0;
    return push_device_impl(d, device_samples, n, false);
}

int adsb_push_device_final(adsb_decoder *d, const void *device_samples, size_t n)
{
    return push_device_impl(d, device_samples, n, true);
}

long adsb_decode_device(adsb_decoder *d, const void *device_samples, size_t n, const adsb_frame **frames)
{
    if (!d || !frames)
        return -1;
    if (adsb_reset(d) != 0 || push_device_impl(d, device_samples, n, true) != 0)
        return -1;
    return (long)d->res.take(frames);
}

int adsb_push_device_packed(adsb_decoder *d, const void *device_packed, size_t n)
{
    if (!d)
        return -1;
    return push_device_packed_impl(d, device_packed, n, false, "adsb_push_device_packed");
}

int adsb_push_device_packed_final(adsb_decoder *d, const void *device_packed, size_t n)
{
    if (!d)
        return -1;
    return push_device_packed_impl(d, device_packed, n, true, "adsb_push_device_packed_final");
}

long adsb_decode_device_packed(adsb_decoder *d, const void *device_packed, size_t n, const adsb_frame **frames)
{
    if (!d || !frames)
        return -1;
    // refused before the reset, at the position the reset will set: a refused call leaves the handle as it was
    if (packed_device_refusal(d, device_packed, n, 0, "adsb_decode_device_packed"))
        return -1;
    if (adsb_reset(d) != 0 || push_device_packed_impl(d, device_packed, n, true, "adsb_decode_device_packed") != 0)
        return -1;
    return (long)d->res.take(frames);
}

int adsb_unpack_packed12(void *dst_u16, const void *src, size_t n, void *stream)
{
    char why[160] = "";
    if (n % adsb::kPackedGroupSamples != 0)
        snprintf(why, sizeof why, "adsb_unpack_packed12: n = %zu is not a multiple of 8", n);
    else if (n && (!dst_u16 || !src))
        snprintf(why, sizeof why, "adsb_unpack_packed12: NULL buffer");
    else if ((uintptr_t)dst_u16 % 16 != 0 || (uintptr_t)src % 4 != 0)
        snprintf(why, sizeof why, "adsb_unpack_packed12: dst must be 16-byte and src 4-byte aligned (%p, %p)", dst_u16, src);
    else if (n) {
        const hipError_t e = adsb::launch_unpack12(static_cast<uint16_t *>(dst_u16), src, n / adsb::kPackedGroupSamples,
                                                   static_cast<hipStream_t>(stream));
        if (e != hipSuccess)
            snprintf(why, sizeof why, "adsb_unpack_packed12: launch failed: %s", hipGetErrorString(e));
    }
    if (!why[0])
        return 0;
    set_create_error(why);
    return -1;
}

size_t adsb_format_bytes(int fmt, size_t n)
{
    const size_t elem = adsb::format_element_bytes(fmt);
    return (elem ? elem : (fmt == adsb::kFmtUint16Real || fmt == adsb::kFmtRaw) ? sizeof(uint16_t) : 0) * n;
}

int adsb_push_as(adsb_decoder *d, int fmt, const void *samples, size_t n)
{
    size_t elem;
    if (!d)
        return -1;
    const int k = format_dispatch(d, "adsb_push_as", fmt, &elem);
    return k < 0 ? -1 : k ? adsb_push(d, static_cast<const uint16_t *>(samples), n) : push_host(d, samples, n, false, false, "adsb_push_as", fmt);
}

int adsb_push_async_as(adsb_decoder *d, int fmt, const void *samples, size_t n)
{
    size_t elem;
    if (!d)
        return -1;
    const int k = format_dispatch(d, "adsb_push_async_as", fmt, &elem);
    return k < 0 ? -1 : k ? adsb_push_async(d, static_cast<const uint16_t *>(samples), n) : push_host(d, samples, n, true, false, "adsb_push_async_as", fmt);
}

int adsb_push_device_as(adsb_decoder *d, int fmt, const void *device_samples, size_t n)
{
    size_t elem;
    if (!d)
        return -1;
    const int k = format_dispatch(d, "adsb_push_device_as", fmt, &elem);
    return k < 0 ? -1 : k ? adsb_push_device(d, device_samples, n) : push_device_as_impl(d, fmt, device_samples, n, false, "adsb_push_device_as");
}

int adsb_push_device_final_as(adsb_decoder *d, int fmt, const void *device_samples, size_t n)
{
    size_t elem;
    if (!d)
        return -1;
    const int k = format_dispatch(d, "adsb_push_device_final_as", fmt, &elem);
    return k < 0 ? -1 : k ? adsb_push_device_final(d, device_samples, n) : push_device_as_impl(d, fmt, device_samples, n, true, "adsb_push_device_final_as");
}

long adsb_decode_device_as(adsb_decoder *d, int fmt, const void *device_samples, size_t n, const adsb_frame **frames)
{
    const char *what = "adsb_decode_device_as";
    size_t elem;
    if (!d || !frames)
        return -1;
    const int k = format_dispatch(d, what, fmt, &elem);
    if (k < 0)
        return -1;
    if (k)
        return adsb_decode_device(d, device_samples, n, frames);
    // refused before the reset: a refused call leaves the handle as it was
    if (device_as_refusal(d, what, device_samples, n, elem))
        return -1;
    if (!d->long_stream && (uint64_t)n >= (1ull << 32)) {
        stream_too_long(d, n);
        return -1;
    }
    if (adsb_reset(d) != 0 || push_device_as_impl(d, fmt, device_samples, n, true, what) != 0)
        return -1;
    return (long)d->res.take(frames);
}

int adsb_get_format_report(const adsb_decoder *d, adsb_format_report *out)
{
    if (!d || !out)
        return -1;
    adsb_decoder *m = const_cast<adsb_decoder *>(d); // the counters live on the device until asked for
    unsigned long long c[2];
    if (format_counters(m, c))
        return -1;
    out->converted = d->fmt_converted;
    out->inexact = c[0] - d->fmt_base[0];
    out->clamped = c[1] - d->fmt_base[1];
    return 0;
}

int adsb_convert_samples(void *dst_u16, const void *src, int fmt, size_t n, uint64_t *device_counters2, void *stream)
{
    char why[200] = "";
    const size_t elem = adsb::format_element_bytes(fmt);
    if (!elem)
        snprintf(why, sizeof why, "adsb_convert_samples: format %d is not converted (1 FLOAT32_REAL, 3 INT16_REAL)", fmt);
    else if (n && (!dst_u16 || !src))
        snprintf(why, sizeof why, "adsb_convert_samples: NULL buffer");
    else if ((uintptr_t)dst_u16 % 2 != 0 || (uintptr_t)src % elem != 0 || (uintptr_t)device_counters2 % 8 != 0)
        snprintf(why, sizeof why, "adsb_convert_samples: dst must be 2-byte, src %zu-byte and the counters 8-byte aligned (%p, %p, %p)", elem,
                 dst_u16, src, (void *)device_counters2);
    else if (n) {
        const hipError_t e = adsb::launch_convert(fmt, static_cast<uint16_t *>(dst_u16), src, n,
                                                  reinterpret_cast<unsigned long long *>(device_counters2), static_cast<hipStream_t>(stream));
        if (e != hipSuccess)
            snprintf(why, sizeof why, "adsb_convert_samples: launch failed: %s", hipGetErrorString(e));
    }
    if (!why[0])
        return 0;
    set_create_error(why);
    return -1;
}

int adsb_count_tries_alone(const uint32_t *tries, uint32_t n_tries, const uint32_t *regions, const uint32_t *region_counts,
                           uint32_t n_tiles, int passes, uint32_t big_tiles, uint64_t g_base, const uint64_t *carry_in,
                           const uint32_t *n_carry, const adsb_try_frame *frames, uint32_t n_frames, uint64_t hi, int final,
                           uint64_t *carry_out, uint32_t carry_cap, uint32_t *n_carry_out, uint32_t *n_carry_next, uint64_t *acc,
                           void *stream)
{
    static_assert(sizeof(adsb_try_frame) == sizeof(adsb::TryFrame) && offsetof(adsb_try_frame, span) == offsetof(adsb::TryFrame, span),
                  "adsb_try_frame is TryFrame");
    char why[240] = "";
    const bool have_regions = regions || region_counts;
    auto off = [](const void *p, size_t a) { return (uintptr_t)p % a != 0; };
    if (!n_carry || !n_carry_out || !n_carry_next || !acc)
        snprintf(why, sizeof why, "adsb_count_tries_alone: NULL n_carry, n_carry_out, n_carry_next or acc");
    else if ((n_tries && !tries) || (n_frames && !frames) || (carry_cap && (!carry_in || !carry_out)) ||
             (have_regions && (!regions || !region_counts)) || (n_tiles && !have_regions))
        snprintf(why, sizeof why, "adsb_count_tries_alone: NULL buffer with a non-zero count (tries %u, tiles %u, frames %u, carry_cap %u)",
                 n_tries, n_tiles, n_frames, carry_cap);
    else if (off(tries, 4) || off(regions, 4) || off(region_counts, 4) || off(n_carry, 4) || off(n_carry_out, 4) || off(n_carry_next, 4) ||
             off(carry_in, 8) || off(carry_out, 8) || off(frames, 8) || off(acc, 8))
        snprintf(why, sizeof why, "adsb_count_tries_alone: the 32-bit arrays must be 4-byte, the 64-bit arrays and the frames 8-byte aligned");
    else if (passes < 2 || passes > adsb::kMaxPasses)
        snprintf(why, sizeof why, "adsb_count_tries_alone: passes = %d is outside 2..%d", passes, adsb::kMaxPasses);
    else if (carry_cap == 0 && !final)
        snprintf(why, sizeof why, "adsb_count_tries_alone: carry_cap == 0 needs final (undecided tries have nowhere to go)");
    else {
        adsb::TryCountArgs a{};
        a.tries = tries;
        a.n_tries = n_tries;
        a.regions = have_regions ? regions : nullptr;
        a.region_counts = have_regions ? region_counts : nullptr;
        a.n_tiles = have_regions ? n_tiles : 0;
        a.passes = passes;
        a.big_tiles = big_tiles;
        a.g_base = g_base;
        a.carry_in = carry_in;
        a.n_carry = n_carry;
        a.frames = reinterpret_cast<const adsb::TryFrame *>(frames);
        a.n_frames = n_frames;
        a.hi = hi;
        a.final = final ? 1 : 0;
        a.carry_out = carry_out;
        a.carry_cap = carry_cap;
        a.n_carry_out = n_carry_out;
        a.n_carry_next = n_carry_next;
        a.acc = reinterpret_cast<unsigned long long *>(acc);
        const hipError_t e = adsb::launch_count_tries(a, static_cast<hipStream_t>(stream));
        if (e != hipSuccess)
            snprintf(why, sizeof why, "adsb_count_tries_alone: launch failed: %s", hipGetErrorString(e));
    }
    if (!why[0])
        return 0;
    set_create_error(why);
    return -1;
}

int adsb_finish(adsb_decoder *d)
{
    if (!d)
        return -1;
    if (d->finished)
        return 0;
    if (d->shard_on)
        return d->fail("a shard stream ends with adsb_shard_end");
    HIP_TRY(d, hipSetDevice(d->device));
    if (process_stage(d, true))
        return -1;
    if (d->cfg.collect_stats && count_tries_pass(d, nullptr, nullptr, nullptr, 0, 0, true))
        return -1; // tries beyond the final position are never visited
    if (wait_last_copy(d)) // the contract of adsb_push_async: every borrowed buffer is free when adsb_finish returns,
        return -1;         // also when the last piece launched no scan that would have implied it
    d->finished = true;
    return 0;
}

long adsb_drain(adsb_decoder *d, adsb_frame *out, size_t cap)
{
    if (!d || (!out && cap))
        return -1;
    return (long)d->res.drain(out, cap);
}

long adsb_take(adsb_decoder *d, const adsb_frame **frames)
{
    if (!d || !frames)
        return -1;
    return (long)d->res.take(frames);
}

size_t adsb_pending(const adsb_decoder *d)
{
    return d ? d->res.pending() : 0;
}

int adsb_get_stats(const adsb_decoder *d, adsb_stats *out)
{
    if (!d || !out)
        return -1;
    adsb_decoder *m = const_cast<adsb_decoder *>(d); // the try counters live on the device until asked for
    if (d->batch_stats_on) { // a batch counts on the host, per capture: the sum
        *out = d->batch_stats;
        return 0;
    }
    if (m->cfg.collect_stats && (hipSetDevice(m->device) != hipSuccess || read_tries(m)))
        return -1;
    *out = m->res.stats();
    return 0;
}

int adsb_get_profile_sized(const adsb_decoder *d, adsb_profile *out, size_t size)
{
    if (!d || !out || size < offsetof(adsb_profile, offsets))
        return -1;
    adsb_decoder *m = const_cast<adsb_decoder *>(d); // kernel times are read from their events on demand
    for (auto &sl : m->slots)
        for (int pair = 0; pair < 2; pair++)
            if (slot_settle_profile(m, sl, pair))
                return -1;
    adsb_profile p = d->prof;
    // the threads of the handle's own that exist at this moment (they are started by the first launch behind a dense one,
    // or by adsb_create when cfg.host_threads asks for them, and live until adsb_destroy): none under ordinary traffic
    p.host_threads_running = (d->reader ? 1u : 0u) + (d->gang ? (uint32_t)d->gang->helpers() : 0u);
    std::memcpy(out, &p, std::min(size, sizeof p));
    return 0;
}

// ---- diagnostics: the power samples of ONE seam launch (adsbdec_amd_diag.h) ----
long adsb_seam_power(adsb_decoder *d, const void *device_samples, uint64_t first_sample, size_t n, uint64_t P, uint64_t g_begin,
                     uint64_t g_end, float *power, size_t power_cap)
{
    if (!d || !device_samples || !power)
        return -1;
    if (!d->long_stream || !d->seam_out)
        return d->fail("adsb_seam_power: the handle was not given adsb_set_long_stream");
    if (P == 0 || P % adsb::kEpoch != 0 || g_begin >= g_end || g_begin < adsb::seam_first(P) || g_end > adsb::seam_end(P))
        return d->fail("adsb_seam_power: [g_begin, g_end) must be a range of the seam offsets [P - %d, P + %d) of a wrap P = w * 2^31, w >= 1",
                       adsb::kSeamWindow, adsb::kSeamBehind);
    if (first_sample % 8 || (uintptr_t)device_samples % 16 || n > (1ull << 62))
        return d->fail("adsb_seam_power: buffer must start at a multiple of 8 samples, 16-byte aligned");
    const size_t n_pow = (size_t)(g_end - g_begin) - 1 + adsb::kSeamWindow;
    if (power_cap < n_pow)
        return d->fail("adsb_seam_power: the launch has %zu power samples, the array holds %zu", n_pow, power_cap);
    HIP_TRY(d, hipSetDevice(d->device));
    if (scan_drain(d))
        return -1;
    if (slot_order_behind_count(d, d->seam_slot, d->stream)) // (a count pass may still read seam_out)
        return -1;
    adsb::Buf<float, adsb::Mem::Pinned> pw;
    HIP_TRY(d, pw.reserve(n_pow));
    adsb::SeamArgs a = seam_args(d, static_cast<const uint16_t *>(device_samples), first_sample, n, P, g_begin, g_end);
    a.want_tries = 0;
    a.power_out = pw;
    HIP_TRY(d, adsb::launch_seam(a, d->stream));
    HIP_TRY(d, hipEventRecord(d->seam_slot.ev_ready[0], d->stream));
    WAIT_EVENT(d, d->seam_slot.ev_ready[0], "a seam launch");
    std::memcpy(power, pw.p, n_pow * sizeof(float));
    return (long)n_pow;
}

} // extern "C"
