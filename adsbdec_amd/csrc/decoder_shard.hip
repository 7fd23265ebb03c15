// decoder_shard.hip -- the shard calls of the multi-GPU driver (multi.cpp): a range of a stream's offsets scanned
// by a handle of its own, the records handed back or resolved in chain mode.  (The handle: decoder_state.hpp.)
#include "decoder_state.hpp"
#include "seam_kernel.h"

using namespace adsb;

namespace {

// what a shard's resolver knows when its chain has reached g_end (chain mode): into the head
void fill_shard_head(adsb_decoder *d, adsb_shard_head *head, uint64_t g_begin, uint64_t g_end, uint64_t head_end, size_t n_frames,
                     size_t bases_cap)
{
    head->g_begin = g_begin;
    head->g_end = g_end;
    head->n_frames = n_frames;
    head->n_head = d->shard_hv.size();
    head->head_end = head_end;
    head->skipped = d->res.skipped();
    if (bases_cap) { // (more bases than the caller's array holds: the stitcher must not use it)
        head->n_bases = d->res.walk_bases() <= bases_cap ? d->res.walk_bases() : 0;
        head->walk_final = d->res.walk_final() ? 1 : 0;
    }
    const adsb_stats &st = d->res.stats();
    for (int k = 0; k < 3; k++)
        head->ok[k] = st.ok[k];
    head->fixed = st.fixed;
}

// the shard's own Try count (collect_stats): every try of [g_begin, g_end) against the speculative frames, on the device
int shard_tries(adsb_decoder *d, adsb_shard_head *head)
{
    if (!d->cfg.collect_stats)
        return 0;
    if (count_tries_pass(d, nullptr, nullptr, nullptr, 0, 0, true) || read_tries(d))
        return -1;
    head->has_tries = 1;
    for (int k = 0; k < 3; k++)
        head->tries[k] = d->res.stats().try_[k];
    return 0;
}

// A flush handle (adsb_set_flush) decodes a stream's end as its silent twin's; a shard or a chain window has no end of its own.
int flush_refusal(adsb_decoder *d, const char *what)
{
    if (!d->flush)
        return 0;
    return d->fail("%s: the handle was given adsb_set_flush, which ends a stream of its own past the reference's horizon; the shard and chain "
                   "primitives scan windows of somebody else's stream (adsb_set_flush(d, 0) on a reset handle, or a handle of its own)", what);
}

// What a shard scan asks of its window in HBM, before anything of the handle changes.
int shard_window_refusal(adsb_decoder *d, const char *what, const void *device_samples, uint64_t first_sample, size_t n,
                         uint64_t g_begin, uint64_t g_end, uint64_t total_samples)
{
    if (flush_refusal(d, what) || shard_too_long(d, what, first_sample, n, total_samples))
        return -1;
    if (first_sample % 8 || (uintptr_t)device_samples % 16)
        return d->fail("%s: buffer must start at a multiple of 8 samples, 16-byte aligned", what);
    if (g_begin % 28)
        return d->fail("%s: g_begin must be a multiple of 28", what);
    if (g_end > g_begin) {
        const uint64_t need_lo = g_begin >= 6 ? 2 * (g_begin - 6) : 0;
        const uint64_t need_hi = 2 * (g_end - 1 + ADSB_WINDOW);
        if (first_sample > need_lo || first_sample + n < need_hi)
            return d->fail("%s: buffer does not cover the window of the owned offsets", what);
    }
    return 0;
}

// Scan + chain resolution of a shard that is resident in HBM; the results stay in the handle (resolver queue, shard_hv).
int scan_shard_resolved_core(adsb_decoder *d, const void *device_samples, uint64_t first_sample, size_t n, uint64_t g_begin,
                             uint64_t g_end, uint64_t total_samples, adsb_shard_head *head, const adsb_frame **fp, uint64_t *bases,
                             size_t bases_cap)
{
    std::memset(head, 0, sizeof *head);
    head->status = 1;
    *fp = nullptr;
    if (d->n_samples != 0 || d->res.pending() != 0) // (it runs this handle's own resolver: a stream in progress would be lost)
        return d->fail("adsb_scan_shard_resolved: the handle holds a stream (adsb_reset it, or use a handle of its own)");
    if (shard_window_refusal(d, "adsb_scan_shard_resolved", device_samples, first_sample, n, g_begin, g_end, total_samples))
        return -1;
    HIP_TRY(d, hipSetDevice(d->device));
    if (scan_drain(d))
        return -1;
    const uint64_t head_end = std::min<uint64_t>(g_end, g_begin + d->shard_head); // (tests shrink the window to reach the stitcher's fallback)
    d->sink = ScanSink{};
    d->shard_hv.clear();
    d->res.start_chain(g_begin, head_end, &d->shard_hv);
    const size_t bcap = (bases && bases_cap) ? bases_cap : 0;
    if (bcap) // the shard's own walk of the deqframe calls, advanced beside the chain while the kernel runs
        d->res.start_walk(g_begin, g_end, total_samples, bases, bcap);
    d->alt_next = true;
    int rc = scan_submit(d, static_cast<const uint16_t *>(device_samples), first_sample, n, g_begin, g_end);
    d->alt_next = false;
    if (rc == 0)
        rc = scan_drain(d);
    if (rc)
        return -1;
    d->res.advance(0, g_end);
    if (shard_tries(d, head))
        return -1;
    const size_t nf = d->res.take(fp);
    fill_shard_head(d, head, g_begin, g_end, head_end, nf, bcap);
    head->status = 0;
    return 0;
}

// The stateless scan of a window that its caller has checked: sorted candidates and try words of [g_begin, g_end) into the
// caller's arrays (adsb_scan_shard, adsb_scan_wrap_window).
int scan_window(adsb_decoder *d, const void *device_samples, uint64_t first_sample, size_t n, uint64_t g_begin, uint64_t g_end,
                adsb_candidate *cands, size_t cand_cap, size_t *n_cands, uint64_t *tries, size_t try_cap, size_t *n_tries)
{
    HIP_TRY(d, hipSetDevice(d->device));
    std::vector<adsb_candidate> cv;
    std::vector<uint64_t> tv;
    if (scan_drain(d))
        return -1;
    d->sink.cands = &cv;
    d->sink.tries = &tv;
    d->alt_next = true;
    int rc = scan_submit(d, static_cast<const uint16_t *>(device_samples), first_sample, n, g_begin, g_end);
    d->alt_next = false;
    if (rc == 0)
        rc = scan_drain(d);
    d->sink = ScanSink{};
    if (rc)
        return -1;
    *n_cands = cv.size();
    *n_tries = tv.size();
    if (cv.size() > cand_cap || tv.size() > try_cap)
        return -2;
    if (!cv.empty())
        std::memcpy(cands, cv.data(), cv.size() * sizeof(adsb_candidate));
    if (!tv.empty())
        std::memcpy(tries, tv.data(), tv.size() * sizeof(uint64_t));
    return 0;
}

} // namespace

extern "C" {

// ---- stateless per-shard scan (multi-GPU path) -----------------
int adsb_scan_shard(adsb_decoder *d, const void *device_samples, uint64_t first_sample, size_t n,
                    uint64_t g_begin, uint64_t g_end, adsb_candidate *cands, size_t cand_cap,
                    size_t *n_cands, uint64_t *tries, size_t try_cap, size_t *n_tries)
{
    if (!d || !device_samples || !n_cands || !n_tries)
        return -1;
    if (shard_window_refusal(d, "adsb_scan_shard", device_samples, first_sample, n, g_begin, g_end, 0))
        return -1;
    return scan_window(d, device_samples, first_sample, n, g_begin, g_end, cands, cand_cap, n_cands, tries, try_cap, n_tries);
}

// adsb_scan_shard for a handle with adsb_set_long_stream: a window at absolute stream positions, cut at the wraps as a stream's
// own scan is (scan_submit: the seam kernel for [P - 1196, P + 28), epoch-relative launches on either side).
int adsb_scan_wrap_window(adsb_decoder *d, const void *device_samples, uint64_t first_sample, size_t n, uint64_t g_begin,
                          uint64_t g_end, adsb_candidate *cands, size_t cand_cap, size_t *n_cands, uint64_t *tries, size_t try_cap,
                          size_t *n_tries)
{
    const char *what = "adsb_scan_wrap_window";
    if (!d || !device_samples || !n_cands || !n_tries)
        return -1;
    if (flush_refusal(d, what))
        return -1;
    if (!d->long_stream)
        return d->fail("%s: the handle was not given adsb_set_long_stream (below 2^32 samples: adsb_scan_shard)", what);
    if (first_sample % 8 || (uintptr_t)device_samples % 16)
        return d->fail("%s: buffer must start at a multiple of 8 samples, 16-byte aligned", what);
    if (first_sample > (1ull << 62) || n > (1ull << 62) || g_begin > (1ull << 61) || g_end > (1ull << 61))
        return d->fail("%s: stream position beyond 2^62", what);
    {   // (scannable_end: a stream's pushes cut a seam range anywhere, an epoch's launches at its run boundaries)
        const uint64_t P = round_down(g_begin, adsb::kEpoch), r = g_begin - P;
        const bool in_seam = (P && r < (uint64_t)adsb::kSeamBehind) || r >= adsb::kEpoch - adsb::kSeamWindow;
        if (!in_seam && r % 28)
            return d->fail("%s: g_begin must be a run boundary of its epoch ((g_begin - P) %% 28 == 0, P = w * 2^31) or a seam offset", what);
    }
    if (g_end > g_begin) {
        const uint64_t need_lo = g_begin >= 6 ? 2 * (g_begin - 6) : 0;
        const uint64_t need_hi = 2 * (g_end - 1 + ADSB_WINDOW);
        if (first_sample > need_lo || first_sample + n < need_hi)
            return d->fail("%s: buffer does not cover the window of the owned offsets", what);
    }
    const uint64_t seam_before = d->seam_offsets; // (a stream's count, adsb_get_wraps: this call is no part of a stream)
    const int rc = scan_window(d, device_samples, first_sample, n, g_begin, g_end, cands, cand_cap, n_cands, tries, try_cap, n_tries);
    d->seam_offsets = seam_before;
    return rc;
}

int adsb_scan_shard_host(adsb_decoder *d, const uint16_t *host_samples, uint64_t first_sample, size_t n, uint64_t g_begin,
                         uint64_t g_end, adsb_candidate *cands, size_t cand_cap, size_t *n_cands, uint64_t *tries, size_t try_cap,
                         size_t *n_tries)
{
    if (!d || !host_samples || !n_cands || !n_tries)
        return -1;
    if (flush_refusal(d, "adsb_scan_shard_host") || shard_too_long(d, "adsb_scan_shard_host", first_sample, n, 0))
        return -1;
    // (copied and waited for: the scan's launches may go to either compute stream, and a window is a few hundred KB.  On a
    // copy stream of the handle's: the synchronous hipMemcpy was seen to cost the process ~1 KB of host memory per call
    // that never came back -- tools/soak_probe.py)
    if (window_in(d, host_samples, n, 0))
        return -1;
    return adsb_scan_shard(d, d->win_buf, first_sample, n, g_begin, g_end, cands, cand_cap, n_cands, tries, try_cap, n_tries);
}

// The same scan, resolved on the fly by this handle's own resolver in chain mode (resolver.hpp): the streaming
// hand-off feeds it while the kernel runs, exactly like a stream's scan; the frames come out with shard-local ts.
int adsb_scan_shard_resolved(adsb_decoder *d, const void *device_samples, uint64_t first_sample, size_t n, uint64_t g_begin,
                             uint64_t g_end, adsb_shard_head *head, adsb_frame *frames, size_t frame_cap,
                             adsb_candidate *head_cands, size_t head_cap)
{
    return adsb_scan_shard_resolved_walk(d, device_samples, first_sample, n, g_begin, g_end, 0, head, frames, frame_cap, head_cands,
                                         head_cap, nullptr, 0);
}


int adsb_scan_shard_resolved_walk(adsb_decoder *d, const void *device_samples, uint64_t first_sample, size_t n, uint64_t g_begin,
                                  uint64_t g_end, uint64_t total_samples, adsb_shard_head *head, adsb_frame *frames,
                                  size_t frame_cap, adsb_candidate *head_cands, size_t head_cap, uint64_t *bases,
                                  size_t bases_cap)
{
    if (!d || !device_samples || !head || (frame_cap && !frames) || (head_cap && !head_cands))
        return -1;
    const adsb_frame *fp = nullptr;
    const int rc = scan_shard_resolved_core(d, device_samples, first_sample, n, g_begin, g_end, total_samples, head, &fp, bases, bases_cap);
    bool fit = false;
    if (rc == 0) {
        fit = head->n_frames <= frame_cap && head->n_head <= head_cap;
        if (fit) {
            if (head->n_frames)
                std::memcpy(frames, fp, head->n_frames * sizeof(adsb_frame));
            if (head->n_head)
                std::memcpy(head_cands, d->shard_hv.data(), head->n_head * sizeof(adsb_candidate));
        } else {
            head->status = 1;
        }
    }
    const std::string why = d->err;
    if (adsb_reset(d) != 0) // (the device's Try accumulators start from zero again; the handle is an ordinary one again)
        return -1;
    if (rc) {
        d->err = why;
        return -1;
    }
    return fit ? 0 : -2;
}

int adsb_scan_shard_resolved_take(adsb_decoder *d, const void *device_samples, uint64_t first_sample, size_t n, uint64_t g_begin,
                                  uint64_t g_end, uint64_t total_samples, adsb_shard_head *head, const adsb_frame **frames,
                                  const adsb_candidate **head_cands, uint64_t *bases, size_t bases_cap)
{
    if (!d || !device_samples || !head || !frames || !head_cands)
        return -1;
    *head_cands = nullptr;
    if (adsb_reset(d) != 0) // what the previous call left in the handle (its frames, the Try accumulators) goes now
        return -1;
    if (scan_shard_resolved_core(d, device_samples, first_sample, n, g_begin, g_end, total_samples, head, frames, bases, bases_cap))
        return -1;
    *head_cands = d->shard_hv.empty() ? nullptr : d->shard_hv.data();
    return 0;
}

// ---- a shard fed piecewise: the same chain-mode resolution, driven by the handle's ordinary stream machinery --------------
int adsb_shard_begin(adsb_decoder *d, uint64_t first_sample, uint64_t g_begin, uint64_t g_end, uint64_t total_samples,
                     uint64_t *bases, size_t bases_cap)
{
    if (!d)
        return -1;
    if (flush_refusal(d, "adsb_shard_begin") || shard_too_long(d, "adsb_shard_begin", first_sample, 0, total_samples))
        return -1;
    if (first_sample % 8)
        return d->fail("adsb_shard_begin: first_sample must be a multiple of 8 samples");
    if (g_begin % 28 || g_end < g_begin)
        return d->fail("adsb_shard_begin: g_begin must be a multiple of 28 and g_end >= g_begin");
    if (first_sample > (g_begin >= 6 ? 2 * (g_begin - 6) : 0))
        return d->fail("adsb_shard_begin: the samples must start at least 6 pairs before the first owned offset");
    if (g_end > g_begin && 2 * (g_end - 1 + ADSB_WINDOW) > total_samples)
        return d->fail("adsb_shard_begin: the shard's last window lies beyond the stream");
    if (adsb_reset(d) != 0)
        return -1;
    d->shard_on = true;
    d->shard_g_begin = g_begin;
    d->shard_g_end = g_end;
    d->n_samples = first_sample;
    d->stage_first = first_sample;
    d->g_scanned = g_begin;
    d->shard_hv.clear();
    d->res.start_chain(g_begin, std::min<uint64_t>(g_end, g_begin + d->shard_head), &d->shard_hv);
    d->shard_bases_cap = (bases && bases_cap) ? bases_cap : 0;
    if (d->shard_bases_cap)
        d->res.start_walk(g_begin, g_end, total_samples, bases, bases_cap);
    return 0;
}

int adsb_shard_end(adsb_decoder *d, adsb_shard_head *head, const adsb_frame **frames, const adsb_candidate **head_cands)
{
    if (!d || !head || !frames || !head_cands)
        return -1;
    std::memset(head, 0, sizeof *head);
    head->status = 1;
    *frames = nullptr;
    *head_cands = nullptr;
    if (!d->shard_on)
        return d->fail("adsb_shard_end without adsb_shard_begin");
    const uint64_t g_begin = d->shard_g_begin, g_end = d->shard_g_end;
    if (g_end > g_begin && d->n_samples / 2 < g_end - 1 + ADSB_WINDOW)
        return d->fail("adsb_shard_end: %llu samples of the stream are in, the shard's last window ends at sample %llu",
                       (unsigned long long)d->n_samples, (unsigned long long)(2 * (g_end - 1 + ADSB_WINDOW)));
    HIP_TRY(d, hipSetDevice(d->device));
    if (process_stage(d, true)) // scans what is left, collects everything in flight, runs the chain to g_end
        return -1;
    if (d->g_scanned < g_end)
        return d->fail("internal: shard scanned to %llu of %llu", (unsigned long long)d->g_scanned, (unsigned long long)g_end);
    if (shard_tries(d, head))
        return -1;
    if (wait_last_copy(d)) // every borrowed buffer is free again
        return -1;
    d->finished = true; // (no further push: the next stream or shard starts with adsb_reset / adsb_shard_begin)
    const size_t nf = d->res.take(frames);
    *head_cands = d->shard_hv.empty() ? nullptr : d->shard_hv.data();
    fill_shard_head(d, head, g_begin, g_end, std::min<uint64_t>(g_end, g_begin + d->shard_head), nf, d->shard_bases_cap);
    head->status = 0;
    return 0;
}

} // extern "C"
