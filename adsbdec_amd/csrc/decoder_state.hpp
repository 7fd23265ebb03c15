// decoder_state.hpp -- what the units of the library's host side share (internal): the handle and its launch slots, the
// waits with a deadline, and the functions one unit calls in another.
//   decoder.hip            the stream machinery: staging, launch, count passes; the push calls
//   decoder_collect.hip    the collect of a launch's records, while it runs (the hand-off stream) or after, and its steps
//   decoder_lifecycle.hip  create, destroy, reset; the device, NUMA and pinned-memory helpers
//   decoder_batch.hip      a batch of independent captures (adsb_decode_batch_*)
//   decoder_shard.hip      the shard calls of the multi-GPU driver (adsb_scan_shard*, adsb_shard_begin / _end)
//   decoder_export.hip     the export calls (adsb_power_*): the front end's power samples into an array of the caller's
//   decoder_export_batch.hip  ... of a batch of captures in one launch (adsb_power_batch_*)
//   decoder_level.hip      the level calls (adsb_level_*): a capture's power samples reduced to a report and an envelope
//   decoder_level_batch.hip  the batch level calls (adsb_level_batch_*): the reports of N captures by one launch per sub-batch
//   decoder_level_windows.hip  the window form (adsb_level_windows*): the reports of K consecutive windows of one stream
//   decoder_bursts.hip     the gate behind the envelope (adsb_bursts_*): an envelope's bursts as an ordered table
//   decoder_gather.hip     a capture's bursts as one array (adsb_gather_device): the pieces of a burst table, packed by one launch
//   decoder_gather_pack12.hip  ... of a real capture, packed to 12 bits while they are copied (adsb_gather_pack12_*)
//   decoder_flavour.hip    what a sample flavour is (flavour.hpp): the judgement of a format number, the _iq and _power checks
//   decoder_stage.hip      the staging steps every family calls: samples into unpacked, batch_in, batch_land, batch_unpacked, win_buf, pow_buf
// Every call from one unit into another is made per launch or per API call; what runs per record or per tile is in decoder_collect.hip.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <unistd.h>

#include <emmintrin.h>

#include "../../include/adsbdec_amd_diag.h"
#include "batch.hpp"
#include "config_abi.hpp"
#include "device_mem.hpp"
#include "handoff.hpp"
#include "packed12.h"
#include "resolver.hpp"
#include "sample_format.h"
#include "scan_kernel.h"

#pragma GCC visibility push(hidden)

#include "flavour.hpp" // the stream kinds, power_samples_produced, struct Flavour

namespace adsb {

// The shipped library reads NO environment variable: what a test must be able to force is a member of adsb_config
// (debug_*).  Builds with -DADSB_TUNING (tools/build_variant.sh; never the one in adsbdec_amd/lib) keep a few knobs for
// A/B runs and diagnosis: ADSB_CHUNK_MI, ADSB_ALT_STREAMS, ADSB_DEBUG_HOST, ADSB_DEBUG_TIMELINE, ADSB_DEBUG_ASYNC.
#ifdef ADSB_TUNING
inline const char *tuning_env(const char *name) { return getenv(name); }
#else
inline const char *tuning_env(const char *) { return nullptr; }
#endif

constexpr uint64_t kDefaultStageSamples = 32ull << 20; // 64 MiB per staging buffer
constexpr uint64_t kStageSlack = 4096;                 // samples kept free for alignment padding
constexpr size_t kInPlaceMinSamples = 1u << 16;
constexpr size_t kSeamSamples = 4096; // > 2*(28+8+1196): enough for the first in-place tile's pre-halo
constexpr int kSlots = 4;
constexpr size_t kTryStateBytes = 4 * sizeof(unsigned long long) + 4 * sizeof(uint32_t); // d_try_acc + d_carry_n
constexpr uint32_t kCarryCap = 1u << 20; // undecided tries carried between count passes (a few hundred in practice)

inline uint64_t round_down(uint64_t v, uint64_t q) { return v - v % q; }

} // namespace adsb

// A launch as what comes behind it sees it -- its completion events, its arguments, and the count pass over its tries
// (count_tries_pass): all that a seam launch has (adsb_decoder::seam_slot), and the head of a scan slot.
struct ScanLaunch {
    int ev_cur = 0;            // copy of the launch in flight
    adsb::Event ev_ready[2];   // the kernel has completed (report and loose list are in)
    adsb::Event ev_count;      // statistics runs: the count pass over the launch's tries (count stream) has ended;
    bool count_pending = false; // the slot's next scan waits for it before it overwrites the list
    bool try_regions = false;  // the launch in flight uses the regions
    uint32_t ntiles = 0;       // tiles of the launch in flight
    adsb::ScanArgs args{};
};

// One scan in flight: the kernel of a chunk of offsets writes its records straight into
// this slot's PINNED HOST buffers (the records are tens of bytes per frame; PCIe writes
// are free next to the sample traffic) -- no device-to-host copy of records, ever.
//   counters   adsb::kDevCounterWords dwords per launch slot, every counter on a cache line of its own
//              and in pinned host memory, written by the kernel
//   cands      "loose" list, kCandWords dwords per record, appended with one atomic: records
//              that could not go through the stream; collected after completion
//   tries      try words of per-shard scans, which hand the list back to the caller
//   d_tries    one dword per DF-gate pass (collect_stats of a stream: counted on the device, on a
//              count stream of its own): a region of kTryRegion words per tile + a launch-wide list
//   hand       the hand-off stream: a marker + the kept records of every tile (scan_kernel.h),
//              consumed while the kernel runs
struct ScanSlot : ScanLaunch {
    adsb::Buf<uint32_t> d_counters; // device: adsb::kDevCounterWords (ScanArgs::counters)
    adsb::Buf<uint32_t, adsb::Mem::PinnedCoherent> h_counters; // written by the launch's report kernel (ScanArgs::report): two
                                    // copies used in turn (ev_cur), so that a launch's kernel time can be read
                                    // behind the slot's NEXT launch instead of in front of it
    adsb::Buf<uint32_t, adsb::Mem::Pinned> cands; // written by the kernel
    adsb::Buf<uint32_t, adsb::Mem::Pinned> tries; // written by the kernel (per-shard scans that return the list); tries.cap words
    adsb::Buf<uint32_t> d_tries;    // device: statistics runs of a stream count tries on the device
    size_t cand_cap = 0, d_try_cap = 0; // records `cands` holds; words of d_tries' launch-wide list
    // d_tries = [d_try_tiles regions of adsb::kTryRegion words][launch-wide list of d_try_cap words]; a tile's
    // whole-tile round writes its region and d_try_counts[tile] (scan_kernel.h), the list takes the rest
    adsb::Buf<uint32_t> d_try_counts;
    size_t d_try_tiles = 0;
    bool tries_on_device = false;   // which of the two the launch in flight uses
    uint64_t ev_offsets[2] = {0, 0}; // offsets of the launch each copy belongs to
    uint32_t *hc() { return h_counters + ev_cur * adsb::kCounterWords; }
    // streaming hand-off (scan_kernel.h): one stream of self-validating granules; fine-grained (coherent), so that the host
    // sees the device's stores while the kernel is still running
    adsb::Buf<uint32_t, adsb::Mem::PinnedCoherent> hand;
    size_t hand_cap = 0;   // granules hand can hold
    bool streaming = false;
    bool busy = false;
    uint64_t piece = 0; // adsb_push_async: the launch belongs to this push piece (collected one piece later)
    hipStream_t launch_stream = nullptr; // where the launch in flight (or the slot's last one) was enqueued
    bool prof_pending[2] = {false, false}; // kernel time of a collected launch not read yet
    uint64_t epoch_base = 0; // long streams: first power sample P of the epoch the launch lies in.  `args` stays in stream
                             // coordinates for everything the host does; the KERNEL is given them minus P (slot_launch)
};

struct ScanSink { // where collected records go: a caller's vectors, or (null) the stream's resolver
    std::vector<adsb_candidate> *cands = nullptr;
    std::vector<uint64_t> *tries = nullptr;
};

// The handle.  Its device resources are members that free themselves (device_mem.hpp), declared so that the streams go
// LAST: behind the buffers and events that were used on them.
//
// Data layout in HBM (decoder_stage.hip is where land[] of a batch -- batch_land --, unpacked, batch_in, batch_unpacked, win_buf and pow_buf
// are filled; land[] of a host push is filled by push_copy in decoder.hip, beside the staging buffers it feeds)
//   stage[2]   uint16 samples; the current one holds stream samples
//              [stage_first, stage_first+stage_fill): what has not been dropped yet plus the
//              newest push (pushes are appended; the scanned part is dropped -- the tail moved to
//              the other buffer -- when the buffer is half full).  stage_first is a multiple of
//              8 samples so that pair index/4 alignment and 16-byte loads line up with the stream.
//              adsb_push_async copies into it on two copy streams of its own (push_copy).
//              (An int8 IQ stream's units are bytes: stage_first, stage_fill and stage_cap count them, and the buffers are half used.)
//              Ordering rule of the copies into it: two writers that are not ordered never share a
//              cache line (process_stage, push_copy).
//   slots[]    the record buffers of the launches in flight (ScanSlot)
//   seam_out   long streams (adsb_set_long_stream): the records and try words of a seam launch (seam_kernel.h), waited for
// A buffer pushed with adsb_push_device() at a stream position that is a multiple
// of 8 samples and a 16-byte aligned address is scanned IN PLACE: only the ~4 KiB
// seam with the previous push and the ~5 KiB tail go through the staging buffer.
// Packed 12-bit input (adsb_push_packed*, adsb_push_device_packed*) is unpacked by a kernel of its own
// (unpack12.hip) into exactly the samples those two paths would have been given as uint16:
//   land[2]    host pushes: the packed bytes of a piece land here (one buffer per copy stream, 1.5 B x
//              stage_cap), and the unpack writes stage[cur] + stage_fill on the stream of that copy
//   unpacked   device pushes: 2 B x n of scratch, scanned in place like a uint16 push
// Signed 16-bit and float32 real input (the _as calls) takes the same two roads through convert_samples.hip: host pushes land in
// land[] (2 B or 4 B x stage_cap each) and are converted into stage[cur] + stage_fill, device pushes are converted into `unpacked`;
// a batch is converted into batch_unpacked by one launch (its table: unpack_tab; _host: the captures land in batch_land).
//   d_fmt      two counters the conversions add to: samples off their format's grid (inexact), and clamped ones
// A batch of captures (adsb_decode_batch_*, batch.hpp) is scanned in place too, by launches of scan_batch_kernel:
//   batch_tab  a launch's segment table and its tile -> segment words (scan_kernel.h BatchSeg), uploaded from its pinned half
//   batch_in   adsb_decode_batch_host: the captures, each at a 128-byte boundary
// and a batch of PACKED captures (adsb_decode_batch_*_packed) is unpacked first, by one launch of unpack12_batch.hip:
//   batch_land     _host_packed: the packed bytes of the captures (1.5 B per sample), each at a 16-byte boundary
//   batch_unpacked the unpacked captures (2 B per sample), each at a 128-byte boundary: what the batch scan then reads
//   unpack_tab     that launch's table, a row per capture that has groups (packed12.h Unpack12Seg), uploaded from its pinned half
struct adsb_decoder {
    adsb_config cfg{};
    adsb_debug_config dbg{}; // the test knobs, copied at adsb_create (adsb_config.debug)
    int device = 0;
    std::string err;
    adsb::Stream stream; // the scan stream: the library's own, or cfg.stream
    // A second compute stream: the launches of a multi-launch IN-PLACE scan (adsb_push_device*, adsb_scan_shard*)
    // alternate between the two, so that launch k+1's first tiles fill the slots launch k's last tiles leave empty
    // (a launch drains for about one tile life, ~40 us of falling occupancy; on one stream the next launch cannot
    // start before the previous one -- and the report kernel behind it -- has ended).  Staged scans stay on `stream`,
    // behind their copies.  A caller-supplied cfg.stream turns it off.
    adsb::Stream stream2;
    adsb::Stream count_stream; // statistics runs: frame uploads + count kernels (count_tries_pass)
    // adsb_push_async: host-to-device copies run on streams of their own, used in turn (measured
    // with rocprofv3 --memory-copy-trace: two copies queued on ONE stream start ~15 us apart,
    // whatever their size -- at the reference's 2 MiB per call that is a quarter of the link;
    // on alternating streams the next copy starts while the previous one is still running)
    static constexpr int kCopyStreams = 2;
    adsb::Stream copy_stream[kCopyStreams];
    bool alt_next = false; // scan_submit: the launches being submitted may alternate

    // stream position
    uint64_t n_samples = 0; // samples accepted
    uint64_t g_scanned = 0; // every offset below has been submitted to the device
    bool finished = false;
    // What the stream holds, fixed by its first push with samples after adsb_create / adsb_reset: real samples (the uint16,
    // packed and _as calls: the FIR front end), complex ones (the _iq calls: scan_iq_kernel.hip) or float32 power samples (the
    // _power calls: scan_power_kernel.hip), or complex int8 ones (the _iq calls with fmt 8: scan_iq8_kernel.hip).  They never mix.
    int kind = adsb::kKindNone;
    // Long streams (adsb_set_long_stream): no refusal at 2^32 samples; launches are cut at every wrap of the reference's
    // sample counter and the offsets around it go through the seam kernel (scan_submit, seam_kernel.h)
    bool long_stream = false;
    // Flush (adsb_set_flush; DESIGN.md "Flush"): a stream's end is decoded as its silent twin's -- the last launch owns every
    // offset up to the last power sample, and the resolver's end is adsb::stream_end(true, ...).  Sticky across adsb_reset.
    bool flush = false;
    uint64_t seam_offsets = 0;    // offsets of the current stream that went through the seam kernel
    adsb::Buf<uint32_t, adsb::Mem::Pinned> seam_out; // adsb::kSeamOutWords (the seam kernel's records and try words)
    ScanLaunch seam_slot;          // the seam launch: its completion event (ev_ready[0]), and its count pass's

    // staging
    adsb::Buf<uint16_t> stage[2];
    int cur = 0;
    uint64_t stage_cap = 0;   // samples per staging buffer
    uint64_t stage_first = 0; // stream index of stage[cur][0]
    uint64_t stage_fill = 0;  // samples held
    bool copy_unconfirmed = false; // a copy of caller's samples has been enqueued on the scan stream and no scan
                                   // launched behind it has been collected yet (the caller's buffer is still in use)

    adsb::Buf<uint32_t> d_synd; // 14 x 256 CRC-24 syndrome table (scan_kernel.h)
    adsb::Buf<uint32_t> d_fix;  // single-bit syndrome hash (extension, cfg.fix_1bit)
    uint32_t fix_mul = 0;
    int n_cus = 256;
    ScanSlot slots[adsb::kSlots];
    int slot_head = 0, slot_count = 0; // FIFO of busy slots
    ScanSink sink;                     // sink of the scans in flight

    adsb_profile prof{};
    adsb::Resolver res;
    std::vector<uint32_t> order, scratch_a, scratch_b, tile_start, tile_count;
    adsb::FinishScratch finish_scratch; // a launch that is finished after completion (handoff.hpp)
    adsb::StreamReader *reader = nullptr;    // the thread that reads the hand-off stream (decoder_collect.hip): cfg.host_threads = 2
                                             // from the start, 0 (auto) from the first launch that follows a dense one
    bool reader_failed = false;              // no thread could be had: do not try again
    adsb::FormatGang *gang = nullptr;        // the threads that write the frames of dense launches (gang.hpp): cfg.host_threads >= 3, or auto
    bool gang_failed = false;
    int gang_l3 = -1;
    uint32_t reader_min_tiles = 1024; // launches below this many tiles are collected by the calling thread alone
    uint64_t last_launch_records = 0; // records the previous launch handed over (auto: the thread pays from kAutoReaderRecords on)
    uint64_t last_launch_offsets = 0; // ... out of this many offsets
    bool no_streaming = false; // dbg.no_streaming: always collect after completion
    uint64_t shard_head = ADSB_SHARD_HEAD; // offsets of a resolved shard whose candidates are ALL kept for the stitcher (dbg.shard_head)
    int dbg_async = 0;         // tuning builds only (ADSB_DEBUG_ASYNC, tools/async_race.py): 1 = wait for every async copy,
                               // 2 = copies on the scan stream, 4 = tail copies not ordered before the next copy (the old race)
    // device-side visited-try count (scan_kernel.h TryCountArgs)
    adsb::Buf<uint64_t> d_carry[2];
    uint32_t *d_carry_n = nullptr; // device: three counts in rotation (in, out, next: TryCountArgs), behind d_try_acc's four
    int carry_n_cur = 0;
    bool carry_maybe = false;      // a non-final pass has run since the last final one: its carry may be non-empty
    int carry_cur = 0;
    adsb::Buf<adsb::TryFrame> d_frames;
    size_t frames_cap = 0;
    adsb::Buf<unsigned long long> d_try_acc; // device, kTryStateBytes: visited tries per DF code since reset + overflow flag,
                                             // then d_carry_n
    bool tries_unread = false;               // passes have been enqueued since the statistics were last read
    bool acc_dirty = false;                  // ... since d_try_acc was last zeroed
    // pinned upload buffers, three in rotation: the resolver logs the frames it accepts straight into one ([0] is kept
    // for the last frame of the pass before), the pass being prepared uploads from the second, the third may still be
    // in flight -- so preparing a pass copies nothing and never waits for an upload
    static constexpr int kFrameBufs = 3;
    adsb::Buf<adsb::TryFrame, adsb::Mem::Pinned> h_frames[kFrameBufs];
    adsb::Event ev_frames[kFrameBufs];
    int log_buf = 0; // the buffer the resolver is logging into
    bool frames_pending[kFrameBufs] = {false, false, false};
    bool final_follows = false;   // adsb_push_device_final: the end-of-stream count pass comes next
    uint32_t deferred_n = 0;
    ScanSlot *deferred_slot = nullptr;
    // A count pass that has been prepared (frames in h_frames[b], arguments fixed) but not enqueued yet: its HIP
    // calls (~14 us of host time) are made right BEHIND the next scan launch instead of in front of it
    // (count_flush), or when the statistics are asked for.  An adsb_reset in between queues its clearing of the
    // accumulators behind it.
    struct PendingCount {
        bool valid = false, clear_after = false;
        adsb::TryCountArgs a{};
        size_t nf = 0;
        int b = 0;
        const adsb::TryFrame *src = nullptr; // first frame to upload (h_frames[b], or one further without a previous frame)
        ScanLaunch *slot = nullptr; // records its ev_count
        hipEvent_t after = nullptr; // the scan (and the report kernel behind it) whose tries the pass reads
    } pending;
    uint64_t deferred_base = 0;
    bool have_prev_frame = false; // last accepted frame of earlier passes (its span may cover later tries)
    uint64_t prev_frame_g = 0;
    uint32_t prev_frame_span = 0;
    uint32_t launch_gen = 0;   // makes every launch's hand-off tags distinct
    adsb::Event ev_copy[kCopyStreams];
    adsb::Event ev_tail; // behind a staging compaction's tail copy (process_stage): the copy streams wait for it
    adsb::Event ev_wait; // wait_stream's marker (created at its first use)
    uint64_t piece = 0;        // pieces pushed asynchronously so far
    // packed 12-bit ingress: landing buffers of host pushes (allocated at the first one), the device pushes' scratch
    adsb::Buf<uint8_t> land[kCopyStreams];
    adsb::Buf<uint16_t> unpacked;  // unpacked.cap samples
    adsb::Event ev_unpack;         // behind a device push's unpack: the second scan stream waits for it
    // converted formats (adsb_*_as): the device's counters run on for the life of the handle; adsb_reset notes where they stand
    adsb::Buf<unsigned long long> d_fmt; // {inexact, clamped}, allocated by the first _as call that converts
    uint64_t fmt_converted = 0;          // samples converted since adsb_create / adsb_reset
    unsigned long long fmt_base[2] = {0, 0};
    bool fmt_dirty = false;              // a conversion has been enqueued since fmt_base was read

    // Shard-stream mode (adsb_shard_begin .. adsb_shard_end): the stream starts at sample shard_first instead of 0, ends
    // behind offset shard_g_end instead of at the end-of-file horizon, and the resolver runs in chain mode.
    bool shard_on = false;
    uint64_t shard_g_begin = 0, shard_g_end = 0;
    size_t shard_bases_cap = 0;
    std::vector<adsb_candidate> shard_hv; // head candidates (handed out in place by adsb_shard_end)
    // A batch of independent captures (adsb_decode_batch_*, batch.hpp): a resolver of its own, reset per capture, and the
    // frames of the whole batch, handed out in place; the handle's stream (res, the staging buffers) stays reset beside it
    adsb::Resolver batch_res;
    std::vector<adsb_frame> batch_frames;
    std::vector<adsb_batch_segment> batch_segs;
    std::vector<adsb_batch_launch> batch_launches;
    std::vector<adsb_candidate> batch_cands, batch_cbuf; // the batch's sorted records in virtual offsets; one capture's
    std::vector<uint64_t> batch_tries, batch_tbuf;
    std::vector<adsb_stats> batch_per;
    adsb::Table batch_tab, unpack_tab;
    adsb::Table export_tab; // adsb_power_batch_*: the export launch's table, a row per capture that has power samples (power_export_batch.hpp)
    adsb::Buf<uint8_t> batch_in, batch_land; // .cap bytes
    adsb::Buf<uint16_t> batch_unpacked;      // .cap samples
    // the last packed or converted batch call: every capture's first sample in batch_unpacked, then the end (for a converted IQ
    // batch a sample is an int16 scalar); empty behind a batch call that fills no such table
    std::vector<size_t> batch_unpacked_at;
    bool batch_stats_on = false; // the last call was a batch: adsb_get_stats answers batch_stats, the sum over its captures
    adsb_stats batch_stats{};
    adsb::Buf<uint16_t> win_buf; // adsb_scan_shard_host, adsb_power_window_host: device copy of the caller's window
    adsb::Buf<float> pow_buf;    // adsb_power_window_host: the window's power samples, copied back from here
    // the level calls (adsb_level_*, decoder_level.hip): the report's words as the kernels add to them (level.h kLevelWords), zeroed on
    // the scan stream at the start of a call and copied to the pinned half before it returns; measurement builds: a row per workgroup
    adsb::Totals<unsigned long long> level;
    adsb::Buf<uint32_t> level_rows;
    // the batch level calls (adsb_level_batch_*, decoder_level_batch.hip): the launch's table, a row per capture that has power samples
    // (level_batch.hpp), and the totals of a sub-batch, kLevelWords per row -- 16 MiB on the device and as much pinned at
    // kLevelBatchCaptures rows, grown to the largest sub-batch seen
    adsb::Table level_tab;
    adsb::Totals<unsigned long long> level_batch;
    int level_batch_blocks = 0; // adsb_debug_set_level_batch_blocks: 0, or the most workgroups a batch level launch may have
    // the gate behind the envelope (adsb_bursts_*, decoder_bursts.hip; burst.h): every tile's summary and, behind them, its combine
    // row; B as the combine leaves it and its pinned twin; the device table of min(B, cap) records.  Grown to the largest call seen.
    // adsb_bursts_slice_* use the same three: the table with one more record, the last burst's, whose copy lands in the pinned
    // words 4 .. 7 behind B.
    adsb::Buf<uint32_t> burst_scratch;
    adsb::Totals<uint32_t> burst_total;
    adsb::Buf<uint32_t> burst_tab;
    // a capture's bursts as one array (adsb_gather_device, decoder_gather.hip; gather.h): the row table of one call, filled in the
    // pinned half and uploaded on the scan stream
    adsb::Table gather_tab;
    // ... packed to 12 bits (adsb_gather_pack12_*, decoder_gather_pack12.hip; gather_pack12.h): the pieces' own samples above 4095, one
    // word the kernel adds to, zeroed on the scan stream in front of the launch and copied to its pinned twin behind it
    adsb::Totals<unsigned long long> gather_over;

    int fail(const char *fmt, ...)
    {
        char buf[512];
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(buf, sizeof buf, fmt, ap);
        va_end(ap);
        err = buf;
        return -1;
    }
};

#define HIP_TRY(d, call)                                                                      \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess)                                                                 \
            return (d)->fail("%s failed: %s (%s:%d)", #call, hipGetErrorString(e_), __FILE__, \
                             __LINE__);                                                       \
    } while (0)

namespace adsb {

// Every wait for the device inside the library has a deadline (cfg.wait_timeout_s, default 120 s): a kernel or copy that never
// completes -- a wedged queue, a device that has gone away -- ends the call with -1 and a message that says what was waited
// for, instead of a host thread that never returns (the reference's counterpart is a read() that cannot hang).  Polls with
// pauses for the first ~200 us (the usual case: the work is microseconds from its end), then sleeps between looks.
template <class Query>
int wait_until_done(adsb_decoder *d, Query &&query, const char *what)
{
    using clk = std::chrono::steady_clock;
    hipError_t q;
    for (int spin = 0; spin < 4096; spin++) {
        if ((q = query()) != hipErrorNotReady)
            goto out;
        _mm_pause(); // (x86-64 only by handoff.hpp's #error: this file includes it)
    }
    {
        const auto t0 = clk::now();
        const auto limit = std::chrono::seconds(d->cfg.wait_timeout_s > 0 ? d->cfg.wait_timeout_s : 120);
        unsigned nap_us = 20;
        for (;;) {
            for (int spin = 0; spin < 256; spin++) {
                if ((q = query()) != hipErrorNotReady)
                    goto out;
                _mm_pause(); // (x86-64 only by handoff.hpp's #error: this file includes it)
            }
            if (clk::now() - t0 > limit)
                return d->fail("the device did not finish %s within %lld s (wedged queue or lost device?): giving up", what,
                               (long long)limit.count());
            if (clk::now() - t0 > std::chrono::milliseconds(2)) { // long waits (copies of GiBs, first-touch page faults) sleep between looks
                usleep(nap_us);
                nap_us = std::min(nap_us * 2, 200u);
            }
        }
    }
out:
    if (q != hipSuccess)
        return d->fail("waiting for %s failed: %s", what, hipGetErrorString(q));
    return 0;
}
inline int wait_event(adsb_decoder *d, hipEvent_t ev, const char *what)
{
#ifdef ADSB_BLOCKING_WAITS // (A/B builds: the runtime's own blocking waits, as until round 4)
    const hipError_t e = hipEventSynchronize(ev);
    return e == hipSuccess ? 0 : d->fail("waiting for %s failed: %s", what, hipGetErrorString(e));
#endif
    return wait_until_done(d, [ev] { return hipEventQuery(ev); }, what);
}
// "Everything enqueued on st so far": ONE marker (an event recorded behind it) and polls of that event.  Not polls of
// hipStreamQuery: each of those has the runtime enqueue a marker of its own while the stream is busy, and a statistics step,
// which waits for its count pass this way once per call, got 6 % slower for it (profiles/r5_ab_runs.txt section 5).
inline int wait_stream(adsb_decoder *d, hipStream_t st, const char *what)
{
#ifdef ADSB_BLOCKING_WAITS
    const hipError_t es = hipStreamSynchronize(st);
    return es == hipSuccess ? 0 : d->fail("waiting for %s failed: %s", what, hipGetErrorString(es));
#endif
    if (!d->ev_wait && d->ev_wait.create(hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        return wait_until_done(d, [st] { return hipStreamQuery(st); }, what);
    }
    // (an idle stream -- most of the streams adsb_reset and adsb_finish wait for -- answers the first question; a marker
    // recorded on an idle stream would cost a round trip to the device, five of them per adsb_reset: measured, +9 % on the
    // statistics step)
    const hipError_t q = hipStreamQuery(st);
    if (q == hipSuccess)
        return 0;
    if (q != hipErrorNotReady)
        return d->fail("waiting for %s failed: %s", what, hipGetErrorString(q));
    const hipError_t e = hipEventRecord(d->ev_wait, st);
    if (e != hipSuccess)
        return d->fail("hipEventRecord (waiting for %s) failed: %s", what, hipGetErrorString(e));
    return wait_event(d, d->ev_wait, what);
}
#define WAIT_EVENT(d, ev, what)   do { if (adsb::wait_event((d), (ev), (what))) return -1; } while (0)
#define WAIT_STREAM(d, st, what)  do { if (adsb::wait_stream((d), (st), (what))) return -1; } while (0)

// Did the previous launch of this handle hand over a record per 2 048 offsets or more (and 16 384 at least)?  The traffic of a
// channel does not change from one launch to the next: the host side starts its helper threads on this (decoder_collect.hip
// choose_helpers), and the next launch takes tiles of six passes instead of seven (adsb::choose_passes).
constexpr uint64_t kAutoReaderRecords = 65536, kAutoReaderMinRecords = 16384;
inline bool last_launch_was_dense(const adsb_decoder *d)
{
    const uint64_t dense_from = std::max<uint64_t>(kAutoReaderMinRecords, std::min<uint64_t>(kAutoReaderRecords, d->last_launch_offsets / 2048));
    return d->last_launch_records >= dense_from;
}

// ---- what one unit calls in another, each per launch or per API call ----
// decoder.hip
int scan_submit(adsb_decoder *d, const uint16_t *buf, uint64_t buf_first, uint64_t buf_n, uint64_t g_begin, uint64_t g_end);
int slot_reserve(adsb_decoder *d, ScanSlot &s, size_t want_cands, size_t want_tries);
int slot_reserve_device_tries(adsb_decoder *d, ScanSlot &s, size_t want_list, size_t want_tiles);
int slot_settle_profile(adsb_decoder *d, ScanSlot &s, int copy);
int slot_order_behind_count(adsb_decoder *d, ScanLaunch &s, hipStream_t st);
int slot_begin_launch(adsb_decoder *d, ScanSlot &s, hipStream_t ls, uint64_t offsets);
int slot_launch(adsb_decoder *d, ScanSlot &s);
void fill_scan_args(const adsb_decoder *d, ScanArgs &a);
void scan_record_room(const adsb_decoder *d, uint64_t n_offsets, size_t *cand_want, size_t *try_want);
int count_flush(adsb_decoder *d);
int count_tries_pass(adsb_decoder *d, ScanLaunch *slot, const uint32_t *tries, const uint32_t *try_counts, uint32_t n_tries,
                     uint64_t g_base, bool final);
int read_tries(adsb_decoder *d);
int process_stage(adsb_decoder *d, bool final, bool in_flight = false);
int wait_last_copy(adsb_decoder *d);
bool stream_too_long(adsb_decoder *d, size_t n);
int format_prepare(adsb_decoder *d, const char *what, size_t land_bytes);
int format_counters(adsb_decoder *d, unsigned long long out[2]);
int kind_refusal(adsb_decoder *d, const char *what, int kind);
bool shard_too_long(adsb_decoder *d, const char *what, uint64_t first_sample, uint64_t n, uint64_t total_samples);
// decoder_collect.hip
int slot_collect(adsb_decoder *d);
int scan_drain(adsb_decoder *d);
void sort_order(adsb_decoder *d, const uint32_t *recs, size_t n);
void sort_tries(adsb_decoder *d, uint32_t *t, size_t n);
void deliver(adsb_decoder *d, const ScanLaunch &s, const uint32_t *recs, const uint32_t *order, size_t nc, int words, int off,
             const uint32_t *tries, size_t nt, uint64_t g_complete);
void book_launch(adsb_decoder *d, ScanSlot &s, uint64_t offsets);
int regrow_if_overflowed(adsb_decoder *d, ScanSlot &s, int attempt);
void start_reader(adsb_decoder *d);
void start_gang(adsb_decoder *d, int helpers);
// decoder_stage.hip: the staging steps (conv = 0: packed 12-bit input is unpacked; else the conversion of sample_format.h)
int to_scratch(adsb_decoder *d, const char *what, int conv, const void *src, size_t n);
int scratch_before_stream2(adsb_decoder *d);
const void *flavour_to_scratch(adsb_decoder *d, const char *what, const Flavour &F, const void *src, size_t n);
enum class Land { InTurnWaited, FirstCopyStream }; // the copy streams in turn, all waited for | copy_stream[0] in order, not waited for
int land_captures(adsb_decoder *d, const char *what, Buf<uint8_t> &buf, const char *of, size_t n_captures, const void *const *src,
                  const size_t *bytes, size_t align, Land how, std::vector<const void *> &at);
int batch_to_scratch(adsb_decoder *d, const char *what, int conv, size_t n_captures, const void *const *src, const size_t *n,
                     std::vector<const void *> &at);
int flavour_batch_to_scratch(adsb_decoder *d, const char *what, const Flavour &F, size_t n_captures, const void *const *src, const size_t *n,
                             std::vector<const void *> &at);
int batch_realign(adsb_decoder *d, const char *what, size_t n_captures, const size_t *bytes, std::vector<const void *> &at);
int window_in(adsb_decoder *d, const uint16_t *samples, size_t n, size_t floats);
int floats_out(adsb_decoder *d, float *dst, size_t floats);
int pow_slots(adsb_decoder *d, size_t n_captures, const size_t *floats, std::vector<float *> &at);
int pow_slots_out(adsb_decoder *d, size_t n_captures, float *const *dst, const std::vector<float *> &at, const size_t *floats, hipStream_t st);
int batch_samples_refusal(adsb_decoder *d, const char *what, size_t i, const void *src, size_t n, const Flavour &F);
// decoder_lifecycle.hip
void set_create_error(const char *why); // what adsb_last_error(NULL) shows: a call without a handle has failed

} // namespace adsb

#pragma GCC visibility pop
