// decoder_collect.hip -- the collect of a scan launch's records: while the launch runs (the hand-off stream, handoff.hpp), or
// after it has ended (the launch-wide lists; a launch some of whose tiles overflowed into them), and their hand-over to the sink
// -- a caller's vectors or the stream's resolver.  Everything here runs per record or per tile.  The steps a collect is made of
// have names, and the batch collect (decoder_batch.hip) uses those that are the same for it.
#include <new>
#include <thread>

#include <sched.h>

#include "decoder_state.hpp"

using namespace adsb;

#pragma GCC visibility push(hidden)

namespace adsb {

static_assert(adsb::kLooseWords == adsb::kCandWords, "handoff.hpp restates the width of a loose record");

// LSD radix sort of the record indices by their 30-bit g_rel (3 x 10 bits).
void sort_order(adsb_decoder *d, const uint32_t *recs, size_t n)
{
    adsb::order_by_g_rel(recs, n, d->order, d->scratch_a, d->scratch_b);
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
void deliver(adsb_decoder *d, const ScanLaunch &s, const uint32_t *recs, const uint32_t *order, size_t nc, int words, int off,
             const uint32_t *tries, size_t nt, uint64_t g_complete)
{
    d->prof.candidates += nc;
    d->prof.tries += nt;
    if (d->sink.cands) {
        for (size_t i = 0; i < nc; i++) {
            const uint32_t *r = recs + (size_t)order[i] * words + off;
            // (a stream record may stand for the same frame at up to three consecutive offsets: scan_kernel_format.h)
            for (uint32_t k = 0, nk = words == adsb::kGranuleWords ? adsb::rec_copies(r) : 1u; k < nk; k++)
                d->sink.cands->push_back(adsb::record_candidate(r, s.args.g_begin, k));
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

// (the reading side of the hand-off stream -- HandCursor, StreamReader, the consumer loops, the merge of a launch that is
// finished after completion -- is host-only code: handoff.hpp)

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

// ---- the handle's helper threads: who starts them, and where they run --------------------------------------------------------

// The handle's second host thread (handoff.hpp StreamReader), kept on the caller's L3.  cfg.host_threads = 2 starts it with the
// handle; 0 (auto) the first time a launch follows one that handed over kAutoReaderRecords or more -- at the channel's
// capacity one thread needs four times the kernel's time for a launch's records, and reading + checking on one thread while
// the caller resolves takes a quarter off that; under ordinary traffic the thread never exists.
// (kAutoReaderRecords and last_launch_was_dense: decoder_state.hpp -- the next launch's tile geometry goes by the same question)
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

static void place_gang(adsb_decoder *d, int cpu)
{
    for (std::thread &t : d->gang->threads())
        d->gang_l3 = adsb::place_reader_thread(t, cpu);
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
    place_gang(d, sched_getcpu());
}

// The caller may have moved since the threads were placed on `placed_l3`: its CPU if that lies on another L3, else -1.
static int caller_moved_to(int placed_l3)
{
    const int cpu = sched_getcpu();
    const int l3 = adsb::l3_of_cpu(cpu);
    return l3 >= 0 && l3 != placed_l3 ? cpu : -1;
}

constexpr int kAutoGangHelpers = 4; // (measured on the dense capture: profiles/r5_gang_runs.txt)

// Which of the handle's helper threads the collect of launch `s` gets.  On a handle left to itself (cfg.host_threads = 0) the
// first launch behind a dense one starts them.
struct LaunchHelpers {
    bool reader = false, gang = false;
};
static LaunchHelpers choose_helpers(adsb_decoder *d, const ScanSlot &s)
{
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
    LaunchHelpers with;
    // (a batch decided ahead packs an offset relative to the launch's first into 31 bits: chunk_offsets() keeps a launch below
    // 2^30 offsets -- kMaxLaunchOffsets -- and this says so where it matters)
    with.gang = d->gang && !d->sink.cands && (uint64_t)s.args.hand_cap * adsb::kGranuleWords * 4 <= adsb::kDecMaxStreamBytes &&
                s.args.g_end - s.args.g_begin < (1ull << 31) && (d->cfg.host_threads >= 3 || after_dense);
    with.reader = d->reader && s.ntiles >= d->reader_min_tiles && (d->cfg.host_threads >= 2 || after_dense);
    return with;
}

// ---- the streaming collect -----------------------------------------------------------------------------------------------------

// With more hands (gang.hpp) a batch is handed to the resolver LATE: meanwhile one of the gang's threads decides it ahead
// (Resolver::speculate_tiles), and the resolver only takes the decisions over.  A flush is cut into batches of kAheadTiles
// tiles, so that several threads decide side by side and the last batch of a launch is a short one; a batch goes on
// as soon as it has been decided (looked at with every flush), at the latest when kMaxHeld are waiting.
struct AheadQueue {
    static constexpr int kMaxHeld = 12;
    static constexpr uint32_t kAheadTiles = 64;
    adsb_decoder *const d;
    ScanSlot &s;
    uint32_t held[kMaxHeld][2];
    int n_held = 0;

    // Every operation returns the records it handed to the resolver.
    size_t deliver_held(int keep, bool only_ready) // the oldest first, until `keep` are left
    {
        size_t nc = 0;
        int k = 0;
        for (; n_held - k > keep && (!only_ready || d->res.ahead_ready()); k++)
            nc += deliver_tiles(d, s, held[k][0], held[k][1]);
        for (int i = k; i < n_held; i++)
            held[i - k][0] = held[i][0], held[i - k][1] = held[i][1];
        n_held -= k;
        return nc;
    }
    size_t flush(uint32_t from, uint32_t upto) // tiles [from, upto) join the queue; what has been decided goes on
    {
        size_t nc = 0;
        while (from < upto) {
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
        return nc + deliver_held(0, true);
    }
    bool idle_work() const { return n_held && d->res.ahead_ready(); } // batches have been decided while the device is behind
};

// The debug timeline of a streaming collect (tuning builds: ADSB_DEBUG_HOST, ADSB_DEBUG_TIMELINE).
struct CollectDebug {
    using clk = std::chrono::steady_clock;
    const bool on = tuning_env("ADSB_DEBUG_HOST") != nullptr;
    double resolve_us = 0;
    int batches = 0;
    static double us(clk::time_point a, clk::time_point b) { return std::chrono::duration<double, std::micro>(b - a).count(); }
    clk::time_point now() const { return on ? clk::now() : clk::time_point(); }
    void resolved_since(clk::time_point tp) { resolve_us += on ? us(tp, clk::now()) : 0.0; }
};

// What the streaming collect leaves to slot_collect.
struct Streamed {
    bool partial = false;      // tiles from resume_tile on are finished after completion (those below were delivered)
    uint32_t resume_tile = 0;
    uint32_t tiles_in = 0;     // every tile below is in the stream, and d->tile_start / tile_count say where
    bool tries_listed = false; // (statistics runs) some tile's tries are on the launch-wide list: its length comes with the counters
};

// Streaming collect: consume the oldest scan WHILE its kernel is still running, so
// that resolving overlaps the scan.  The hand-off stream (scan_kernel.h) is read strictly
// sequentially -- one prefetchable stream of device-written lines, no directory to poll:
// a marker says which tile follows, how many records, and what their XOR must be; the
// records are checked where they lie (16-byte loads) and later resolved in place.  Tiles
// reserve their ranges in COMPLETION order, so a tile that finished early waits (start and
// count noted) until every tile before it is in; the resolver is fed whenever the device
// leaves the host nothing to read, or a group of tiles has accumulated.
// out.partial if a tile reported records on the loose list (or the stream is full): the
// caller then finishes the launch through the collect-after-completion path, from tile
// out.resume_tile on.
static int slot_collect_streaming(adsb_decoder *d, ScanSlot &s, Streamed &out)
{
    using clk = std::chrono::steady_clock;
    const auto t_begin = clk::now();

    std::vector<uint32_t> &t_start = d->tile_start; // per tile: granule index of its first record ...
    std::vector<uint32_t> &t_count = d->tile_count; // ... and its record count (~0u: not in yet)
    t_start.assign(s.ntiles, 0u);
    t_count.assign(s.ntiles, ~0u);
    uint32_t delivered = 0; // every tile below has been handed to the resolver
    uint64_t recs_handed = 0;
    CollectDebug dbg;
    double wait_ms = 0;
    auto t_last_wait = t_begin;
    AheadQueue ahead{d, s};

    const LaunchHelpers with = choose_helpers(d, s);
    if (d->dbg.gang_min > 0) {
        d->res.set_gang(with.gang ? d->gang : nullptr, (size_t)d->dbg.gang_min);
        d->res.set_ahead_min_records((size_t)d->dbg.gang_min);
    } else {
        d->res.set_gang(with.gang ? d->gang : nullptr);
    }
    if (with.gang) {
        if (const int cpu = caller_moved_to(d->gang_l3); cpu >= 0)
            place_gang(d, cpu);
        d->gang->begin();
        d->prof.gang_launches++;
    }
    auto flush = [&](uint32_t upto) { // tiles [delivered, upto): their ranges, one after the other, are sorted
        const auto tp = dbg.now();
        const size_t nc = with.gang ? ahead.flush(delivered, upto) : deliver_tiles(d, s, delivered, upto);
        delivered = upto;
        recs_handed += nc;
        if (dbg.on) {
            dbg.resolved_since(tp);
            dbg.batches++;
            if (tuning_env("ADSB_DEBUG_TIMELINE"))
                fprintf(stderr, "  t=%.1f us: tiles < %u resolved (%zu records), waited %.1f us so far\n",
                        CollectDebug::us(t_begin, clk::now()), upto, nc, wait_ms * 1e3);
        }
    };
    const adsb::HandJob job = hand_job(s);
    adsb::CollectEnd end;
    if (with.reader) {
        adsb::StreamReader &rd = *d->reader;
        if (const int cpu = rd.place ? caller_moved_to(rd.placed_l3) : -1; cpu >= 0)
            rd.placed_l3 = adsb::place_reader_thread(rd.th, cpu);
        auto idle = [&]() -> bool { // batches that have been decided meanwhile go on while the device is behind
            if (!ahead.idle_work())
                return false;
            const auto tp = dbg.now();
            recs_handed += ahead.deliver_held(0, true);
            dbg.resolved_since(tp);
            return true;
        };
        end = adsb::collect_behind_reader(rd, job, t_start.data(), t_count.data(), delivered, flush, wait_ms, t_last_wait, idle);
        if (dbg.on)
            fprintf(stderr, "stream reader thread: busy %.1f us, waits %.1f us\n", rd.busy_ms * 1e3, rd.wait_ms * 1e3);
    } else {
        end = adsb::collect_alone(job, t_start.data(), t_count.data(), delivered, flush, wait_ms, t_last_wait);
    }
    if (ahead.n_held) { // the batches that were still waiting for their turn
        const auto tp = dbg.now();
        recs_handed += ahead.deliver_held(0, false);
        dbg.resolved_since(tp);
    }
    if (end.status < 0 && with.gang) {
        d->res.sync();
        d->gang->end();
    }
    if (end.status == -1)
        return d->fail("hand-off stream corrupt at granule %u (tile %u twice)", end.pos, end.tile);
    if (end.status == -2)
        return d->fail("scan kernel finished without publishing granule %u (tile %u of %u pending)", end.pos, end.tile, s.ntiles);
    if (with.gang) { // the frames of this launch are whole before its stream is touched again (and before anyone counts the time)
        d->res.sync();
        d->gang->end();
    }
    if (dbg.on) {
        fprintf(stderr, "gang: %s, ahead %d, frames taken over so far %llu\n", with.gang ? "on" : "off", (int)with.gang,
                (unsigned long long)d->res.ahead_taken());
        fprintf(stderr,
                "stream collect: %.1f us in all, resolve %.1f us in %d batches, waits %.1f us; %.1f us after the last wait\n",
                CollectDebug::us(t_begin, clk::now()), dbg.resolve_us, dbg.batches, wait_ms * 1e3, CollectDebug::us(t_last_wait, clk::now()));
    }
    const double total_ms = std::chrono::duration<double, std::milli>(clk::now() - t_begin).count();
    d->prof.wait_ms += wait_ms;
    d->prof.host_ms += total_ms - wait_ms;
    out.partial = end.status == 1;
    out.resume_tile = delivered;
    out.tiles_in = end.frontier;
    out.tries_listed = end.tries_listed;
    d->last_launch_records = recs_handed; // (a launch that is finished after completion adds its part there)
    d->last_launch_offsets = s.args.g_end - s.args.g_begin;
    return 0;
}

// ---- the steps of a collect ------------------------------------------------------------------------------------------------------

// Book a launch of `offsets` offsets that has been collected in the profile; its kernel time is read later (slot_settle_profile).
void book_launch(adsb_decoder *d, ScanSlot &s, uint64_t offsets)
{
    s.prof_pending[s.ev_cur] = d->cfg.profile != 0;
    d->prof.launches++;
    d->prof.offsets += offsets;
    d->prof.last_offsets = offsets;
}

// Did the launch-wide lists hold what the ended launch counted?  0: yes.  1: no, and they have been regrown -- sparse output is
// sized for far more than noise produces; the counters keep counting past the capacity, so one repeat with exact sizes suffices.
int regrow_if_overflowed(adsb_decoder *d, ScanSlot &s, int attempt)
{
    const size_t nc = s.hc()[0], nt = s.hc()[1];
    if (nc <= s.cand_cap && nt <= (s.tries_on_device ? s.d_try_cap : s.tries.cap))
        return 0;
    if (attempt >= 2)
        return d->fail("record buffers overflowed repeatedly (%zu candidates, %zu tries)", nc, nt);
    d->prof.relaunches++;
    WAIT_STREAM(d, s.launch_stream ? s.launch_stream : d->stream, "the launch's stream");
    if (slot_reserve(d, s, std::max(s.cand_cap, nc + nc / 8 + 64), s.tries_on_device ? s.tries.cap : std::max(s.tries.cap, nt + nt / 8 + 64)))
        return -1;
    if (s.tries_on_device && slot_reserve_device_tries(d, s, std::max(s.d_try_cap, nt + nt / 8 + 64), s.d_try_tiles))
        return -1;
    return 1;
}

// Wait for the launch's end and its counters; a launch whose lists overflowed is repeated with lists that hold everything.
// (The batch collect has a loop of its own: it launches inside it.)
static int await_counters(adsb_decoder *d, ScanSlot &s, bool partial, bool *relaunched)
{
    for (int attempt = 0;; attempt++) {
        // (every tile has been consumed: the kernel is ending and its report is microseconds
        // away -- poll for it instead of going to sleep in hipEventSynchronize)
        WAIT_EVENT(d, s.ev_ready[s.ev_cur], s.streaming && !partial ? "the end of a scan launch whose every tile has been consumed" : "a scan launch");
        book_launch(d, s, s.args.g_end - s.args.g_begin);
        if (slot_settle_profile(d, s, s.ev_cur))
            return -1;
        const int again = regrow_if_overflowed(d, s, attempt);
        if (again <= 0)
            return again;
        *relaunched = true;
        if (slot_launch(d, s))
            return -1;
        // the repeat is consumed after completion: tiles below resume_tile (if any)
        // were delivered by the first run and are skipped by the finish below
    }
}

// Statistics runs: the launch's tries (n_listed of them on its launch-wide list) are counted now -- or, the stream's last
// launch, by the end-of-stream pass, which runs right after the final resolver step: one device round trip instead of two.
static int count_or_defer_tries(adsb_decoder *d, ScanSlot &s, uint32_t n_listed)
{
    if (!s.tries_on_device)
        return 0;
    if (d->final_follows && d->slot_count == 1) {
        d->deferred_slot = &s;
        d->deferred_n = n_listed;
        d->deferred_base = s.args.g_begin;
        return 0;
    }
    return count_tries_pass(d, &s, s.d_tries, s.d_try_counts, n_listed, s.args.g_begin, false);
}

static void retire_slot(adsb_decoder *d, ScanSlot &s)
{
    s.busy = false;
    d->slot_head = (d->slot_head + 1) % kSlots;
    d->slot_count--;
}

// Some tile could not put all its records into the hand-off stream: the launch has ended, its loose list is complete, and the
// tiles from st.resume_tile on are handed on by adsb::finish_after_completion (handoff.hpp says how).
static void slot_finish_after_completion(adsb_decoder *d, ScanSlot &s, const Streamed &st, bool relaunched)
{
    d->last_launch_records = std::max<uint64_t>(d->last_launch_records, s.hc()[2] / 2); // (an estimate from the granules the stream used)
    // (the streaming collect went on reading and checking behind the first tile that held it up: when it got to the end
    // of the launch, where every tile's records lie is known already)
    const bool walked = st.tiles_in == s.ntiles && !relaunched;
    if (!walked) {
        // Every granule that was ever written is in: walk the stream again from its start.  Whatever ends the walk -- a missing
        // marker, one that does not fit, a tile a second time -- the tiles behind it are on the loose list (where corruption is
        // an error, the streaming collect has failed the call).
        d->tile_start.assign(s.ntiles, 0u);
        d->tile_count.assign(s.ntiles, ~0u);
        adsb::HandJob job = hand_job(s);
        job.cap = (uint32_t)std::min<size_t>(s.hc()[2], s.args.hand_cap);
        job.done = nullptr;
        adsb::walk_what_is_there(job, d->tile_start.data(), d->tile_count.data());
    }
    adsb::finish_after_completion(
        s.hand, d->tile_start.data(), d->tile_count.data(), s.ntiles, st.resume_tile, s.args.g_begin, s.args.g_end,
        [&](uint32_t u) { return (uint64_t)adsb::kRun * adsb::tile_first_run(u, s.args.big_tiles, s.args.passes); }, s.cands, s.hc()[0],
        d->finish_scratch, [&](uint32_t from, uint32_t upto) { deliver_tiles(d, s, from, upto); },
        [&](const uint32_t *recs, size_t n, uint64_t g_complete) {
            d->order.resize(n);
            for (size_t i = 0; i < n; i++)
                d->order[i] = (uint32_t)i;
            deliver(d, s, recs, d->order.data(), n, adsb::kCandWords, 0, nullptr, 0, g_complete);
        });
}

// Wait for the oldest scan in flight and hand its records on, in ascending g.
int slot_collect(adsb_decoder *d)
{
    ScanSlot &s = d->slots[d->slot_head];
    using clk = std::chrono::steady_clock;
    Streamed st;
    if (s.streaming && slot_collect_streaming(d, s, st))
        return -1;
    if (s.streaming && !st.partial && !st.tries_listed && (!s.tries_on_device || s.try_regions)) {
        // Every tile has been published and consumed and none used the loose list -- nor, in a statistics
        // run, the launch-wide try list: a tile that overflows its survivor queue says so in its marker (kMarkTries:
        // its records are in the stream and have been handed on like any other's), and the tries of all others are
        // in their regions.  The launch-wide counters have nothing to add, so
        // do not wait for them (nor for the kernel's end event -- the profile reads that later).
        book_launch(d, s, s.args.g_end - s.args.g_begin);
        if (count_or_defer_tries(d, s, 0))
            return -1;
        retire_slot(d, s);
        return 0;
    }
    const auto t_wait = clk::now();
    bool relaunched = false;
    if (await_counters(d, s, st.partial, &relaunched))
        return -1;
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
    } else if (st.partial) {
        slot_finish_after_completion(d, s, st, relaunched);
    } else if (nc != 0) {
        return d->fail("internal: %zu loose records without a tile overflow flag", nc);
    }
    if (count_or_defer_tries(d, s, (uint32_t)nt))
        return -1;
    d->res.sync(); // (tiles handed on after completion may have gone to the gang as well)
    if (d->gang)
        d->gang->end(); // ... and FormatGang::post() begins the gang again by itself: without this the helpers would poll on until
                        // the next launch that goes through the gang -- under traffic that has turned sparse, until adsb_destroy
    d->prof.host_ms += std::chrono::duration<double, std::milli>(clk::now() - t_host).count();
    retire_slot(d, s);
    return 0;
}

int scan_drain(adsb_decoder *d)
{
    while (d->slot_count)
        if (slot_collect(d))
            return -1;
    return 0;
}

} // namespace adsb

#pragma GCC visibility pop
