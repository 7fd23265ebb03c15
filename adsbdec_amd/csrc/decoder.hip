// decoder.hip -- the stream machinery of libadsbdec_amd.so's host side: device staging, kernel launches, the collect of a
// launch's records (while it runs, or after), the count passes, and the C-ABI calls of include/adsbdec_amd.h that push,
// finish and read a stream.  Everything that runs per record or per tile is here; the handle itself and the units beside
// this one: decoder_state.hpp.
#include <new>
#include <thread>

#include <sched.h>

#include "decoder_state.hpp"
#include "packed12.h"
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

static int slot_reserve_device_tries(adsb_decoder *d, ScanSlot &s, size_t want_list, size_t want_tiles)
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

static int slot_launch(adsb_decoder *d, ScanSlot &s)
{
    const bool stats = d->cfg.collect_stats != 0;
    s.ev_cur ^= 1;
    if (slot_settle_profile(d, s, s.ev_cur)) // two launches old: normally read long ago
        return -1;
    s.ev_offsets[s.ev_cur] = s.args.g_end - s.args.g_begin;
    s.ntiles = adsb::tile_count(s.args.g_end - s.args.g_begin, s.args.big_tiles, s.args.passes);
    // A stream's statistics run keeps the try words on the device (counted there after
    // resolution); a per-shard scan hands the list back, sorted, so it needs the list
    // complete on the host: collect after completion.
    s.tries_on_device = stats && !d->sink.cands;
    s.streaming = !d->no_streaming && (!stats || s.tries_on_device);
    s.args.gen = ++d->launch_gen * 0x9E3779B9u + 0x7F4A7C15u;
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
    s.args.counters = s.d_counters;
    s.args.cands = s.cands;
    s.args.cand_cap = (uint32_t)std::min<size_t>(s.cand_cap, 0xFFFFFFFFu);
    const int slot_index = (int)(&s - d->slots);
    hipStream_t ls = (d->alt_next && d->stream2 && (slot_index & 1)) ? d->stream2.st : d->stream.st;
    if (s.launch_stream && s.launch_stream != ls) // the slot's previous launch (its report kernel zeroes the counters) ran on the other stream
        HIP_TRY(d, hipStreamWaitEvent(ls, s.ev_ready[s.ev_cur ^ 1], 0));
    s.launch_stream = ls;
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
    // d_counters are zero here: cleared at creation, and the report kernel behind every scan leaves them so
    s.args.profile = d->cfg.profile ? 1 : 0;
    s.args.report = s.hc();
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

// LSD radix sort of the record indices by their 30-bit g_rel (3 x 10 bits).
void sort_order(adsb_decoder *d, const uint32_t *recs, size_t n)
{
    d->order.resize(n);
    d->scratch_a.resize(n);
    d->scratch_b.resize(n);
    uint32_t *idx = d->order.data(), *tmp = d->scratch_a.data(), *key = d->scratch_b.data();
    bool sorted = true;
    for (size_t i = 0; i < n; i++) {
        idx[i] = (uint32_t)i;
        key[i] = recs[i * adsb::kCandWords];
        if (i && key[i] < key[i - 1])
            sorted = false;
    }
    if (sorted)
        return;
    for (int shift = 0; shift < 30; shift += 10) {
        uint32_t hist[1025] = {0};
        for (size_t i = 0; i < n; i++)
            hist[((key[idx[i]] >> shift) & 1023u) + 1]++;
        for (int b = 0; b < 1024; b++)
            hist[b + 1] += hist[b];
        for (size_t i = 0; i < n; i++)
            tmp[hist[(key[idx[i]] >> shift) & 1023u]++] = idx[i];
        std::swap(idx, tmp);
    }
    if (idx != d->order.data())
        std::memcpy(d->order.data(), idx, n * sizeof(uint32_t)); // odd number of passes
}

void sort_tries(adsb_decoder *d, uint32_t *t, size_t n)
{
    bool sorted = true;
    for (size_t i = 1; i < n && sorted; i++)
        sorted = t[i] >= t[i - 1];
    if (sorted)
        return;
    d->scratch_a.resize(n);
    uint32_t *src = t, *dst = d->scratch_a.data();
    for (int shift = 0; shift < 32; shift += 11) {
        uint32_t hist[2049] = {0};
        for (size_t i = 0; i < n; i++)
            hist[((src[i] >> shift) & 2047u) + 1]++;
        for (int b = 0; b < 2048; b++)
            hist[b + 1] += hist[b];
        for (size_t i = 0; i < n; i++)
            dst[hist[(src[i] >> shift) & 2047u]++] = src[i];
        std::swap(src, dst);
    }
    if (src != t)
        std::memcpy(t, src, n * sizeof(uint32_t));
}

// Hand sorted records to the sink (a caller's vectors or the stream's resolver).
// Record i is the 6 dwords {g_rel, pw, frame | len << 16 | flags << 24} at
// recs[order[i] * words + off] (loose list / gathered copy: words 6, off 0; hand-off
// stream consumed in place: words 4 = granule index, off 1).
static void deliver(adsb_decoder *d, const ScanLaunch &s, const uint32_t *recs, const uint32_t *order, size_t nc, int words,
             int off, const uint32_t *tries, size_t nt, uint64_t g_complete)
{
    d->prof.candidates += nc;
    d->prof.tries += nt;
    if (d->sink.cands) {
        for (size_t i = 0; i < nc; i++) {
            const uint32_t *r = recs + (size_t)order[i] * words + off;
            adsb_candidate c;
            std::memset(&c, 0, sizeof c);
            std::memcpy(c.frame, &r[2], 14);
            c.len = (uint8_t)((r[5] >> 16) & 0xFF);
            c.reserved = (uint8_t)((r[5] >> 24) & 1u);
            // (a stream record may stand for the same frame at up to three consecutive offsets: scan_kernel_format.h)
            for (uint32_t k = 0, nk = words == adsb::kGranuleWords ? adsb::rec_copies(r) : 1u; k < nk; k++) {
                c.g = s.args.g_begin + r[0] + k;
                c.pw = k ? r[5 + k] : r[1];
                d->sink.cands->push_back(c);
            }
        }
        for (size_t i = 0; i < nt; i++)
            d->sink.tries->push_back((((uint64_t)(tries[i] >> 2) + s.args.g_begin) << 2) | (tries[i] & 3u));
    } else if (nt == 0) {
        d->res.capture_head(recs, order, nc, words, off, s.args.g_begin);
        d->res.advance_device(recs, order, nc, words, off, s.args.g_begin, power_samples_produced(d->n_samples),
                              g_complete);
    } else {
        d->res.feed_device(recs, order, nc, words, off, s.args.g_begin, tries, nt);
        d->res.advance(power_samples_produced(d->n_samples), g_complete);
    }
}

// (the reading side of the hand-off stream -- HandCursor, StreamReader, the two consumer loops -- is host-only code:
// handoff.hpp)

// "has the launch behind these bytes ended?" for handoff.hpp: ctx is the launch's completion event
static int launch_done(void *ctx)
{
    const hipError_t q = hipEventQuery(static_cast<hipEvent_t>(ctx));
    return q == hipErrorNotReady ? 0 : q == hipSuccess ? 1 : -1;
}

static adsb::HandJob hand_job(const ScanSlot &s)
{
    adsb::HandJob j;
    j.hand = s.hand;
    j.ntiles = s.ntiles;
    j.gen = s.args.gen;
    j.cap = s.args.hand_cap;
    j.done = launch_done;
    j.ctx = s.ev_ready[s.ev_cur];
    return j;
}

// Tiles [from, upto) of the launch's hand-off stream (d->tile_start / d->tile_count say where each one's records lie) go to
// the sink: a caller's vectors, or the stream's resolver, which walks the ranges where they lie.  Returns the records handed on.
static size_t deliver_tiles(adsb_decoder *d, ScanSlot &s, uint32_t from, uint32_t upto)
{
    const uint32_t *t_start = d->tile_start.data(), *t_count = d->tile_count.data();
    const uint64_t g_complete = std::min<uint64_t>(
        s.args.g_end, s.args.g_begin + adsb::kRun * adsb::tile_first_run(upto, s.args.big_tiles, s.args.passes));
    size_t nc = 0;
    if (d->sink.cands) { // per-shard scan: the caller's vectors
        std::vector<uint32_t> &order = d->order; // the records in ascending g (granule indices)
        order.clear();
        for (uint32_t u = from; u < upto; u++)
            for (uint32_t i = 0, b = t_start[u], n = t_count[u]; i < n; i++)
                order.push_back(b + 2 * i);
        nc = order.size();
        deliver(d, s, s.hand, order.data(), nc, adsb::kGranuleWords, 0, nullptr, 0, g_complete);
    } else { // the stream's resolver walks the tile ranges where they lie
        for (uint32_t u = from; u < upto; u++)
            nc += t_count[u];
        d->prof.candidates += nc;
        if (d->res.head_wanted(s.args.g_begin + adsb::kRun * adsb::tile_first_run(from, s.args.big_tiles, s.args.passes)))
            d->res.capture_head_tiles(s.hand, t_start, t_count, from, upto, s.args.g_begin);
        d->res.advance_tiles(s.hand, t_start, t_count, from, upto, s.args.g_begin, power_samples_produced(d->n_samples), g_complete);
    }
    return nc;
}

// Streaming collect: consume the oldest scan WHILE its kernel is still running, so
// that resolving overlaps the scan.  The hand-off stream (scan_kernel.h) is read strictly
// sequentially -- one prefetchable stream of device-written lines, no directory to poll:
// a marker says which tile follows, how many records, and what their XOR must be; the
// records are checked where they lie (16-byte loads) and later resolved in place.  Tiles
// reserve their ranges in COMPLETION order, so a tile that finished early waits (start and
// count noted) until every tile before it is in; the resolver is fed whenever the device
// leaves the host nothing to read, or a group of tiles has accumulated.
// Returns 1 if a tile reported records on the loose list (or the stream is full): the
// caller then finishes the launch through the collect-after-completion path, from tile
// *resume_tile on.
// The handle's second host thread (handoff.hpp StreamReader), kept on the caller's L3.  cfg.host_threads = 2 starts it with the
// handle; 0 (auto) the first time a launch follows one that handed over kAutoReaderRecords or more -- at the channel's
// capacity one thread needs four times the kernel's time for a launch's records, and reading + checking on one thread while
// the caller resolves takes a quarter off that; under ordinary traffic the thread never exists.
constexpr uint64_t kAutoReaderRecords = 65536, kAutoReaderMinRecords = 16384;

// Did the previous launch of this handle hand over a record per 2 048 offsets or more (and 16 384 at least)?  The traffic of a
// channel does not change from one launch to the next: the host side starts its helper threads on this (slot_collect), and the
// next launch takes tiles of six passes instead of seven (adsb::choose_passes).
static inline bool last_launch_was_dense(const adsb_decoder *d)
{
    const uint64_t dense_from = std::max<uint64_t>(kAutoReaderMinRecords, std::min<uint64_t>(kAutoReaderRecords, d->last_launch_offsets / 2048));
    return d->last_launch_records >= dense_from;
}
void start_reader(adsb_decoder *d)
{
    if (d->reader || d->reader_failed)
        return;
    d->reader = new (std::nothrow) adsb::StreamReader;
    if (d->reader) {
        d->reader->on_start = [](void *ctx) { (void)hipSetDevice(static_cast<adsb_decoder *>(ctx)->device); }; // launch_done()
        d->reader->on_start_ctx = d;
        try {
            d->reader->start();
        } catch (...) { // no thread to be had: the calling thread consumes the stream alone, as without the option
            delete d->reader;
            d->reader = nullptr;
        }
    }
    if (d->reader) {
        d->reader->place = true;
        d->reader->placed_l3 = adsb::place_reader_thread(d->reader->th, sched_getcpu());
    } else {
        d->reader_failed = true;
    }
}

// More hands for a channel at its capacity (gang.hpp): the calling thread decides, `helpers` threads on its L3 write the frames.
void start_gang(adsb_decoder *d, int helpers)
{
    if (d->gang || d->gang_failed)
        return;
    d->gang = new (std::nothrow) adsb::FormatGang;
    if (d->gang && !d->gang->start(helpers)) { // no thread to be had: the calling thread writes its frames itself, as without
        delete d->gang;
        d->gang = nullptr;
    }
    if (!d->gang) {
        d->gang_failed = true;
        return;
    }
    const int cpu = sched_getcpu();
    for (std::thread &t : d->gang->threads())
        d->gang_l3 = adsb::place_reader_thread(t, cpu);
}

constexpr int kAutoGangHelpers = 4; // (measured on the dense capture: profiles/r5_gang_runs.txt)

static int slot_collect_streaming(adsb_decoder *d, ScanSlot &s, uint32_t *resume_tile, uint32_t *tiles_in, bool *tries_listed)
{
    using clk = std::chrono::steady_clock;
    const auto t_begin = clk::now();

    std::vector<uint32_t> &t_start = d->tile_start; // per tile: granule index of its first record ...
    std::vector<uint32_t> &t_count = d->tile_count; // ... and its record count (~0u: not in yet)
    t_start.assign(s.ntiles, 0u);
    t_count.assign(s.ntiles, ~0u);
    uint32_t delivered = 0; // every tile below has been handed to the resolver
    uint64_t recs_handed = 0;
    bool overflowed = false;
    double dbg[3] = {0, 0, 0};
    const bool dbg_on = tuning_env("ADSB_DEBUG_HOST") != nullptr;
    double wait_ms = 0;
    auto t_last_wait = t_begin;
    // With more hands (gang.hpp) a batch is handed to the resolver LATE: meanwhile one of the gang's threads decides it ahead
    // (Resolver::speculate_tiles), and the resolver only takes the decisions over.  A flush is cut into batches of kAheadTiles
    // tiles, so that several threads decide side by side and the last batch of a launch is a short one; a batch goes on
    // as soon as it has been decided (looked at with every flush), at the latest when kMaxHeld are waiting.
    constexpr int kMaxHeld = 12;
    constexpr uint32_t kAheadTiles = 64;
    uint32_t held[kMaxHeld][2];
    int n_held = 0;
    bool ahead = false;                    // (set below, once it is known whether this launch goes through the gang)
    auto deliver_held = [&](int keep, bool only_ready) { // the oldest first, until `keep` are left
        size_t nc = 0;
        int k = 0;
        for (; n_held - k > keep && (!only_ready || d->res.ahead_ready()); k++)
            nc += deliver_tiles(d, s, held[k][0], held[k][1]);
        for (int i = k; i < n_held; i++)
            held[i - k][0] = held[i][0], held[i - k][1] = held[i][1];
        n_held -= k;
        return nc;
    };
    auto flush = [&](uint32_t upto) { // tiles [delivered, upto): their ranges, one after the other, are sorted
        clk::time_point tp;
        if (dbg_on)
            tp = clk::now();
        size_t nc = 0;
        if (ahead) {
            for (uint32_t from = delivered; from < upto;) {
                const uint32_t to = std::min(upto, from + kAheadTiles);
                if (n_held == kMaxHeld)
                    nc += deliver_held(kMaxHeld - 1, false);
                if (d->res.speculate_tiles(s.hand, d->tile_start.data(), d->tile_count.data(), from, to, s.args.g_begin)) {
                    held[n_held][0] = from, held[n_held][1] = to;
                    n_held++;
                    d->prof.gang_batches++;
                } else { // (a batch too small to be worth it: in its turn, by this thread)
                    nc += deliver_held(0, false);
                    nc += deliver_tiles(d, s, from, to);
                }
                from = to;
            }
            nc += deliver_held(0, true);
        } else {
            nc += deliver_tiles(d, s, delivered, upto);
        }
        delivered = upto;
        recs_handed += nc;
        if (dbg_on) {
            dbg[1] += std::chrono::duration<double, std::micro>(clk::now() - tp).count();
            dbg[2] += 1;
            if (tuning_env("ADSB_DEBUG_TIMELINE"))
                fprintf(stderr, "  t=%.1f us: tiles < %u resolved (%zu records), waited %.1f us so far\n",
                        std::chrono::duration<double, std::micro>(clk::now() - t_begin).count(), upto, nc, wait_ms * 1e3);
        }
    };
    const adsb::HandJob job = hand_job(s);
    adsb::CollectEnd end;
    // "a channel near its capacity" is a DENSITY: 65 536 records out of a full launch's 128 Mi offsets = one per 2 048 (a full
    // channel has one per 1 090).  Round 6: a shorter launch -- a 128 Mi-sample shard of the multi-GPU driver is 64 Mi offsets,
    // 61 k records on a full channel -- counts by the same density, from 16 384 records on (below that a launch is resolved
    // faster than five threads are woken).
    const bool after_dense = d->cfg.host_threads == 0 && last_launch_was_dense(d);
    if (after_dense) {
        start_reader(d);
        cpu_set_t allowed; // (six threads that poll need cores of their own: on a small or confined host, round 4's pair)
        if (sched_getaffinity(0, sizeof allowed, &allowed) != 0 || CPU_COUNT(&allowed) >= 2 * (kAutoGangHelpers + 2))
            start_gang(d, kAutoGangHelpers);
    }
    // (a batch decided ahead packs an offset relative to the launch's first into 31 bits: chunk_offsets() keeps a launch below
    // 2^30 offsets -- kMaxLaunchOffsets -- and this says so where it matters)
    const bool with_gang = d->gang && !d->sink.cands && (uint64_t)s.args.hand_cap * adsb::kGranuleWords * 4 <= adsb::kDecMaxStreamBytes &&
                           s.args.g_end - s.args.g_begin < (1ull << 31) && (d->cfg.host_threads >= 3 || after_dense);
    if (d->dbg.gang_min > 0) {
        d->res.set_gang(with_gang ? d->gang : nullptr, (size_t)d->dbg.gang_min);
        d->res.set_ahead_min_records((size_t)d->dbg.gang_min);
    } else {
        d->res.set_gang(with_gang ? d->gang : nullptr);
    }
    if (with_gang) {
        const int cpu = sched_getcpu(); // the caller may have moved since the threads were placed
        const int l3 = adsb::l3_of_cpu(cpu);
        if (l3 >= 0 && l3 != d->gang_l3)
            for (std::thread &t : d->gang->threads())
                d->gang_l3 = adsb::place_reader_thread(t, cpu);
        d->gang->begin();
        ahead = true;
        d->prof.gang_launches++;
    }
    if (d->reader && s.ntiles >= d->reader_min_tiles && (d->cfg.host_threads >= 2 || after_dense)) {
        adsb::StreamReader &rd = *d->reader;
        if (rd.place) { // the caller may have moved since the thread was placed
            const int cpu = sched_getcpu();
            const int l3 = adsb::l3_of_cpu(cpu);
            if (l3 >= 0 && l3 != rd.placed_l3)
                rd.placed_l3 = adsb::place_reader_thread(rd.th, cpu);
        }
        auto idle = [&]() -> bool { // batches that have been decided meanwhile go on while the device is behind
            if (!n_held || !d->res.ahead_ready())
                return false;
            clk::time_point tp;
            if (dbg_on)
                tp = clk::now();
            recs_handed += deliver_held(0, true);
            if (dbg_on)
                dbg[1] += std::chrono::duration<double, std::micro>(clk::now() - tp).count();
            return true;
        };
        end = adsb::collect_behind_reader(rd, job, t_start.data(), t_count.data(), delivered, flush, wait_ms, t_last_wait, idle);
        if (dbg_on)
            fprintf(stderr, "stream reader thread: busy %.1f us, waits %.1f us\n", rd.busy_ms * 1e3, rd.wait_ms * 1e3);
    } else {
        end = adsb::collect_alone(job, t_start.data(), t_count.data(), delivered, flush, wait_ms, t_last_wait);
    }
    if (n_held) { // the batches that were still waiting for their turn
        const auto tp = clk::now();
        recs_handed += deliver_held(0, false);
        if (dbg_on)
            dbg[1] += std::chrono::duration<double, std::micro>(clk::now() - tp).count();
    }
    if (end.status < 0 && with_gang) {
        d->res.sync();
        d->gang->end();
    }
    if (end.status == -1)
        return d->fail("hand-off stream corrupt at granule %u (tile %u twice)", end.pos, end.tile);
    if (end.status == -2)
        return d->fail("scan kernel finished without publishing granule %u (tile %u of %u pending)", end.pos, end.tile, s.ntiles);
    overflowed = end.status == 1;
    if (with_gang) { // the frames of this launch are whole before its stream is touched again (and before anyone counts the time)
        d->res.sync();
        d->gang->end();
    }
    if (dbg_on)
        fprintf(stderr, "gang: %s, ahead %d, frames taken over so far %llu\n", with_gang ? "on" : "off", (int)ahead,
                (unsigned long long)d->res.ahead_taken());
    if (dbg_on)
        fprintf(stderr,
                "stream collect: %.1f us in all, resolve %.1f us in %d batches, waits %.1f us; %.1f us after the last wait\n",
                std::chrono::duration<double, std::micro>(clk::now() - t_begin).count(), dbg[1], (int)dbg[2], wait_ms * 1e3,
                std::chrono::duration<double, std::micro>(clk::now() - t_last_wait).count());
    const double total_ms = std::chrono::duration<double, std::milli>(clk::now() - t_begin).count();
    d->prof.wait_ms += wait_ms;
    d->prof.host_ms += total_ms - wait_ms;
    *resume_tile = delivered;
    *tiles_in = end.frontier;
    *tries_listed = end.tries_listed;
    d->last_launch_records = recs_handed; // (a launch that is finished after completion adds its part there)
    d->last_launch_offsets = s.args.g_end - s.args.g_begin;
    return overflowed ? 1 : 0;
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

// Wait for the oldest scan in flight and hand its records on, in ascending g.
static int slot_collect(adsb_decoder *d)
{
    ScanSlot &s = d->slots[d->slot_head];
    using clk = std::chrono::steady_clock;
    uint32_t resume_tile = 0, tiles_in = 0;
    bool partial = false; // tiles below resume_tile were already delivered
    bool relaunched = false;
    bool tries_listed = false; // (statistics runs) some tile's tries are on the launch-wide list: its length comes with the counters
    if (s.streaming) {
        const int rc = slot_collect_streaming(d, s, &resume_tile, &tiles_in, &tries_listed);
        if (rc < 0)
            return -1;
        partial = rc == 1;
    }
    if (s.streaming && !partial && !tries_listed && (!s.tries_on_device || s.try_regions)) {
        // Every tile has been published and consumed and none used the loose list -- nor, in a statistics
        // run, the launch-wide try list: a tile that overflows its survivor queue says so in its marker (kMarkTries:
        // its records are in the stream and have been handed on like any other's), and the tries of all others are
        // in their regions.  The launch-wide counters have nothing to add, so
        // do not wait for them (nor for the kernel's end event -- the profile reads that later).
        s.prof_pending[s.ev_cur] = d->cfg.profile != 0;
        d->prof.launches++;
        d->prof.offsets += s.args.g_end - s.args.g_begin;
        d->prof.last_offsets = s.args.g_end - s.args.g_begin;
        if (s.tries_on_device) {
            if (d->final_follows && d->slot_count == 1) { // (see below)
                d->deferred_slot = &s;
                d->deferred_n = 0;
                d->deferred_base = s.args.g_begin;
            } else if (count_tries_pass(d, &s, s.d_tries, s.d_try_counts, 0, s.args.g_begin, false)) {
                return -1;
            }
        }
        s.busy = false;
        d->slot_head = (d->slot_head + 1) % kSlots;
        d->slot_count--;
        return 0;
    }
    const auto t_wait = clk::now();
    for (int attempt = 0;; attempt++) {
        if (s.streaming && !partial) {
            // every tile has been consumed: the kernel is ending and its report is microseconds
            // away -- poll for it instead of going to sleep in hipEventSynchronize
            WAIT_EVENT(d, s.ev_ready[s.ev_cur], "the end of a scan launch whose every tile has been consumed");
        } else {
            WAIT_EVENT(d, s.ev_ready[s.ev_cur], "a scan launch");
        }
        s.prof_pending[s.ev_cur] = d->cfg.profile != 0;
        if (slot_settle_profile(d, s, s.ev_cur))
            return -1;
        d->prof.launches++;
        d->prof.offsets += s.args.g_end - s.args.g_begin;
        d->prof.last_offsets = s.args.g_end - s.args.g_begin;
        const size_t nc = s.hc()[0], nt = s.hc()[1];
        if (nc <= s.cand_cap && nt <= (s.tries_on_device ? s.d_try_cap : s.tries.cap))
            break;
        // Sparse output sized for far more than noise produces; the counters keep
        // counting past the capacity, so one repeat with exact sizes suffices.
        if (attempt >= 2)
            return d->fail("record buffers overflowed repeatedly (%zu candidates, %zu tries)", nc, nt);
        d->prof.relaunches++;
        relaunched = true;
        WAIT_STREAM(d, s.launch_stream ? s.launch_stream : d->stream, "the launch's stream");
        if (slot_reserve(d, s, std::max(s.cand_cap, nc + nc / 8 + 64),
                         s.tries_on_device ? s.tries.cap : std::max(s.tries.cap, nt + nt / 8 + 64)))
            return -1;
        if (s.tries_on_device && slot_reserve_device_tries(d, s, std::max(s.d_try_cap, nt + nt / 8 + 64), s.d_try_tiles))
            return -1;
        if (slot_launch(d, s))
            return -1;
        // the repeat is consumed after completion: tiles below resume_tile (if any)
        // were delivered by the first run and are skipped by the gather below
    }
    const auto t_host = clk::now();
    d->prof.wait_ms += std::chrono::duration<double, std::milli>(t_host - t_wait).count();
    const size_t nc = s.hc()[0], nt = s.hc()[1];
    if (!s.streaming) {
        // collect-after-completion: everything is in the launch-wide lists, in arrival order
        sort_order(d, s.cands, nc);
        if (nt && !s.tries_on_device)
            sort_tries(d, s.tries, nt);
        const size_t nt_host = s.tries_on_device ? 0 : nt;
        deliver(d, s, s.cands, d->order.data(), nc, adsb::kCandWords, 0, s.tries, nt_host, s.args.g_end);
    } else if (partial) {
        // Some tile could not put all its records into the hand-off stream (staged list or survivor queue overflowed, its
        // range did not fit): those records are on the loose list, which is only complete now that the kernel has ended.
        // Every granule that was ever written is in: walk the stream again from its start (a missing or non-fitting marker
        // ends it), note where each tile's records lie, sort the LOOSE records (few) and hand the tiles on in order -- runs of
        // tiles that are whole in the stream where they lie, like the streaming collect does; a tile with loose records, or
        // none in the stream at all, merged on the way.  (Round 3 gathered and sorted everything that was left: 4 ms for
        // the 311 k records of a dense launch in which ONE early tile had overflowed.)
        std::vector<uint32_t> &t_start = d->tile_start, &t_count = d->tile_count;
        // (the streaming collect went on reading and checking behind the first tile that held it up: when it got to the end
        // of the launch, where every tile's records lie is known already)
        d->last_launch_records = std::max<uint64_t>(d->last_launch_records, s.hc()[2] / 2); // (an estimate from the granules the stream used)
        const bool walked = tiles_in == s.ntiles && !relaunched;
        if (!walked) {
            t_start.assign(s.ntiles, 0u);
            t_count.assign(s.ntiles, ~0u);
        }
        const uint32_t lim = walked ? 0u : (uint32_t)std::min<size_t>(s.hc()[2], s.args.hand_cap);
        for (uint32_t pos = 0; pos < lim;) {
            const uint32_t *m = s.hand + (size_t)pos * adsb::kGranuleWords;
            const uint32_t tile = m[0], nf = m[1], n = nf & 0xFFFFu;
            if (tile >= s.ntiles || (nf & adsb::kMarkNoFit) || (uint64_t)pos + 1 + 2ull * n > lim || t_count[tile] != ~0u)
                break;
            uint32_t a[4] = {0, 0, 0, 0}, sum = 0, lo, hi;
            for (uint32_t k = 0; k < 8 * n; k++)
                a[k & 3] ^= m[4 + k];
            for (uint32_t r = 0; r < n; r++)
                sum += adsb::record_term(r, m[4 + 8 * r], m[5 + 8 * r]);
            adsb::marker_check(tile, nf, s.args.gen, a[0], a[1], a[2], a[3], sum, lo, hi);
            if (m[2] != lo || m[3] != hi)
                break;
            t_start[tile] = pos + 1;
            t_count[tile] = n;
            pos += std::max(adsb::marker_granules(nf), adsb::stream_granules(n));
        }
        // The loose list may also hold records of tiles the streamed part has already delivered: after a relaunch (record
        // buffers regrown) every tile runs again, and whether a tile's range fits the stream depends on completion order.
        const uint64_t resume_rel = (uint64_t)adsb::kRun * adsb::tile_first_run(resume_tile, s.args.big_tiles, s.args.passes);
        d->gather.clear();
        for (size_t i = 0; i < nc; i++) {
            const uint32_t *w = s.cands + i * adsb::kCandWords;
            if (w[0] >= resume_rel)
                d->gather.insert(d->gather.end(), w, w + adsb::kCandWords);
        }
        const size_t n_loose = d->gather.size() / adsb::kCandWords;
        sort_order(d, d->gather.data(), n_loose);
        const std::vector<uint32_t> loose_order(d->order.begin(), d->order.begin() + (ptrdiff_t)n_loose); // (deliver() reuses d->order)
        std::vector<uint32_t> &merged = d->scratch_b; // one tile's records, kCandWords each, ascending
        std::vector<uint32_t> iota;
        size_t li = 0;
        uint32_t run_from = resume_tile;
        for (uint32_t u = resume_tile; u < s.ntiles; u++) {
            const uint64_t hi_rel = (uint64_t)adsb::kRun * adsb::tile_first_run(u + 1, s.args.big_tiles, s.args.passes);
            size_t lj = li;
            while (lj < n_loose && d->gather[(size_t)loose_order[lj] * adsb::kCandWords] < hi_rel)
                lj++;
            if (t_count[u] != ~0u && lj == li)
                continue; // whole in the stream: part of the current run
            if (u > run_from)
                deliver_tiles(d, s, run_from, u);
            // this tile: its records in the stream (if it got that far) merged with its loose ones, both ascending
            merged.clear();
            const uint32_t ns = t_count[u] == ~0u ? 0u : t_count[u];
            const uint32_t *sr = s.hand + (size_t)t_start[u] * adsb::kGranuleWords;
            uint32_t si = 0;
            while (si < ns || li < lj) {
                const uint32_t *lw = li < lj ? d->gather.data() + (size_t)loose_order[li] * adsb::kCandWords : nullptr;
                const uint32_t *sw = si < ns ? sr + (size_t)si * 2 * adsb::kGranuleWords : nullptr;
                if (sw && (!lw || sw[0] <= lw[0])) {
                    // {g_rel, pw, w0, w1}{w2, w3, pw', pw''}: the first six words, once per offset the record stands for (a run
                    // of copies is never interleaved with a loose record: the offsets are consecutive and every offset yields
                    // at most one candidate -- but a loose one may lie INSIDE the run only if it is one of its offsets, which
                    // the tile would have staged with the others; so the run goes in whole)
                    for (uint32_t k = 0, nk = adsb::rec_copies(sw); k < nk; k++) {
                        const uint32_t one[adsb::kCandWords] = {sw[0] + k, k ? sw[5 + k] : sw[1], sw[2], sw[3], sw[4],
                                                                 sw[5] & ~(3u << adsb::kRecCopiesShift)};
                        merged.insert(merged.end(), one, one + adsb::kCandWords);
                    }
                    si++;
                } else {
                    merged.insert(merged.end(), lw, lw + adsb::kCandWords);
                    li++;
                }
            }
            const size_t nm = merged.size() / adsb::kCandWords;
            iota.resize(nm);
            for (size_t i = 0; i < nm; i++)
                iota[i] = (uint32_t)i;
            const uint64_t g_complete = std::min<uint64_t>(s.args.g_end, s.args.g_begin + hi_rel);
            deliver(d, s, merged.data(), iota.data(), nm, adsb::kCandWords, 0, nullptr, 0, g_complete);
            run_from = u + 1;
        }
        if (s.ntiles > run_from)
            deliver_tiles(d, s, run_from, s.ntiles);
    } else if (nc != 0) {
        return d->fail("internal: %zu loose records without a tile overflow flag", nc);
    }
    if (s.tries_on_device) {
        if (d->final_follows && d->slot_count == 1) {
            // last launch of the stream: its tries are counted by the end-of-stream pass, which
            // runs right after the final resolver step -- one device round trip instead of two
            d->deferred_slot = &s;
            d->deferred_n = (uint32_t)nt;
            d->deferred_base = s.args.g_begin;
        } else if (count_tries_pass(d, &s, s.d_tries, s.d_try_counts, (uint32_t)nt, s.args.g_begin, false)) {
            return -1;
        }
    }
    d->res.sync(); // (tiles handed on after completion may have gone to the gang as well)
    if (d->gang)
        d->gang->end(); // ... and FormatGang::post() begins the gang again by itself: without this the helpers would poll on until
                        // the next launch that goes through the gang -- under traffic that has turned sparse, until adsb_destroy
    d->prof.host_ms += std::chrono::duration<double, std::milli>(clk::now() - t_host).count();
    s.busy = false;
    d->slot_head = (d->slot_head + 1) % kSlots;
    d->slot_count--;
    return 0;
}

int scan_drain(adsb_decoder *d)
{
    while (d->slot_count)
        if (slot_collect(d))
            return -1;
    return 0;
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
    a.want_tries = stats ? 1 : 0;
    a.out = d->seam_out;
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
        a.g_begin = g_begin;
        a.g_end = g_stop;
        fill_scan_args(d, a);
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
    const uint64_t m_ref = final ? 2 * ((d->n_samples + 3) / 4) : m_real;
    if (!in_flight) // (in flight: the records below g_scanned are not all in yet; slot_collect advanced as far as they are)
        d->res.advance(m_ref, d->g_scanned);
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
            HIP_TRY(d, adsb::launch_copy_samples(d->stage[d->cur ^ 1], d->stage[d->cur] + skip, left, ts)); // (the library's own kernel:
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
static int push_copy(adsb_decoder *d, const void *src, size_t n, hipMemcpyKind kind, bool async = false, bool packed = false)
{
    const char *p = static_cast<const char *>(src);
    while (n) {
        uint64_t room = d->stage_cap - kStageSlack - d->stage_fill;
        if (packed)
            room = round_down(room, adsb::kPackedGroupSamples);
        if (room == 0)
            return d->fail("staging buffer exhausted (stage_samples too small)");
        const size_t take = (size_t)std::min<uint64_t>(room, n);
        const size_t bytes = packed ? take / adsb::kPackedGroupSamples * adsb::kPackedGroupBytes : take * sizeof(uint16_t);
        if (async) {
            d->piece++;
            const int cs = (int)(d->piece % adsb_decoder::kCopyStreams);
            hipStream_t cstream = d->dbg_async == 2 ? d->stream.st : d->copy_stream[cs].st;
            // Same rule as for the tail copy in process_stage: two writers that are not ordered never share a
            // cache line.  A piece that starts inside a 128-byte line (pushes of odd sizes) waits for the copy of
            // the piece before it, which ends in that line.
            if (d->piece > 1 && (d->stage_fill * sizeof(uint16_t)) % 128 != 0 && d->dbg_async != 2)
                HIP_TRY(d, hipStreamWaitEvent(cstream, d->ev_copy[cs ^ 1], 0));
            if (packed) {
                HIP_TRY(d, hipMemcpyAsync(d->land[cs], p, bytes, kind, cstream));
                HIP_TRY(d, adsb::launch_unpack12(d->stage[d->cur] + d->stage_fill, d->land[cs], take / adsb::kPackedGroupSamples, cstream));
            } else {
                HIP_TRY(d, hipMemcpyAsync(d->stage[d->cur] + d->stage_fill, p, bytes, kind, cstream));
            }
            HIP_TRY(d, hipEventRecord(d->ev_copy[cs], cstream));
            if (d->dbg_async != 2)
                HIP_TRY(d, hipStreamWaitEvent(d->stream, d->ev_copy[cs], 0));
            if (d->dbg_async == 1)
                WAIT_STREAM(d, cstream, "a copy stream");
        } else {
            // (packed: land[0] -- an earlier asynchronous piece that used it is ordered in front by its event, and an earlier
            // synchronous push was complete when it returned)
            if (packed) {
                HIP_TRY(d, hipMemcpyAsync(d->land[0], p, bytes, kind, d->stream));
                HIP_TRY(d, adsb::launch_unpack12(d->stage[d->cur] + d->stage_fill, d->land[0], take / adsb::kPackedGroupSamples, d->stream));
            } else {
                HIP_TRY(d, hipMemcpyAsync(d->stage[d->cur] + d->stage_fill, p, bytes, kind, d->stream));
            }
            d->copy_unconfirmed = true;
        }
        d->stage_fill += take;
        d->n_samples += take;
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

// adsb_push, adsb_push_async and their packed forms: samples in host memory (`packed`: whole groups of 12-bit samples).
static int push_host(adsb_decoder *d, const void *samples, size_t n, bool async, bool packed, const char *what)
{
    if (!d)
        return -1;
    if (d->finished)
        return d->fail("%s after adsb_finish", what);
    if ((packed && packed_refusal(d, what, n, d->n_samples)) || stream_too_long(d, n))
        return -1;
    if (n == 0)
        return 0;
    if (!samples)
        return d->fail("%s: NULL samples", what);
    HIP_TRY(d, hipSetDevice(d->device));
    if (packed) { // the landing buffers, one per copy stream: a handle that never sees packed input has none
        const size_t bytes = d->stage_cap / adsb::kPackedGroupSamples * adsb::kPackedGroupBytes;
        for (auto &l : d->land)
            if (l.reserve(bytes) != hipSuccess) {
                (void)hipGetLastError();
                return d->fail("packed input: cannot allocate a landing buffer of %zu bytes on the device", bytes);
            }
    }
    if (async)
        return push_copy(d, samples, n, hipMemcpyHostToDevice, true, packed);
    if (d->cfg.push_overlap) {
        // The caller's ONE buffer (fileInput's iqbuff, air.c:230-239; the callback's transfer, air.c:173-177) is
        // only borrowed until its bytes are on the device: return when the COPY (packed: copy + unpack) has completed and
        // leave the scan in flight -- the host is back in read() while the device scans, and this call has meanwhile collected
        // the frames of the previous one (frames arrive one call late, never reordered; adsb_finish / adsb_sync
        // deliver the rest).  That is adsb_push_async plus the wait for this piece's own copy.
        if (push_copy(d, samples, n, hipMemcpyHostToDevice, true, packed))
            return -1;
        return wait_last_copy(d);
    }
    if (push_copy(d, samples, n, hipMemcpyHostToDevice, false, packed))
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
static int push_device_impl(adsb_decoder *d, const void *device_samples, size_t n, bool final)
{
    if (!d)
        return -1;
    if (d->finished)
        return d->fail("adsb_push_device after adsb_finish");
    if (final && d->shard_on)
        return d->fail("a shard stream ends with adsb_shard_end");
    if (stream_too_long(d, n))
        return -1;
    if (n && !device_samples)
        return d->fail("adsb_push_device: NULL samples");
    HIP_TRY(d, hipSetDevice(d->device));
    const uint16_t *p = static_cast<const uint16_t *>(device_samples);
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
        d->res.advance(2 * ((total + 3) / 4), d->g_scanned); // EOF rule: see process_stage()
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
    HIP_TRY(d, adsb::launch_copy_samples(d->stage[d->cur], p + (keep_first - first), left, d->stream));
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

static int push_device_packed_impl(adsb_decoder *d, const void *device_packed, size_t n, bool final, const char *what)
{
    if (d->finished)
        return d->fail("%s after adsb_finish", what);
    if (final && d->shard_on)
        return d->fail("a shard stream ends with adsb_shard_end");
    if (packed_device_refusal(d, device_packed, n, d->n_samples, what) || stream_too_long(d, n))
        return -1;
    if (n == 0)
        return final ? push_device_impl(d, nullptr, 0, true) : 0;
    HIP_TRY(d, hipSetDevice(d->device));
    if (d->unpacked.reserve(n) != hipSuccess) { // (every earlier push into the scratch has completed: push_device_impl returns behind its reads)
        (void)hipGetLastError();
        return d->fail("%s: cannot allocate %zu bytes of device scratch for the unpacked samples (2 bytes per sample)", what,
                       n * sizeof(uint16_t));
    }
    HIP_TRY(d, adsb::launch_unpack12(d->unpacked, device_packed, n / adsb::kPackedGroupSamples, d->stream));
    if (d->stream2) { // the in-place launches alternate onto the second scan stream, which nothing else orders behind the unpack
        if (!d->ev_unpack)
            HIP_TRY(d, d->ev_unpack.create(hipEventDisableTiming));
        HIP_TRY(d, hipEventRecord(d->ev_unpack, d->stream));
        HIP_TRY(d, hipStreamWaitEvent(d->stream2, d->ev_unpack, 0));
    }
    return push_device_impl(d, d->unpacked, n, final);
}

} // namespace adsb

extern "C" {

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

} // extern "C"
