// decoder_lifecycle.hip -- a handle's life: adsb_create, adsb_destroy, adsb_reset and the settings made between streams; the
// device, NUMA and pinned-memory helpers; adsb_last_error.  (The handle: decoder_state.hpp.)
#include <new>
#include <thread>

#include "decoder_state.hpp"
#include "seam_kernel.h"

using namespace adsb;

namespace {

thread_local std::string g_create_error;
const char *g_cpu_refusal = nullptr; // set by adsb_create on a host without AVX2 (a plain pointer store: nothing of this file's
                                     // vector code has run by then); adsb_last_error(NULL) shows it

} // namespace

void adsb::set_create_error(const char *why) { g_create_error = why; }

extern "C" {

adsb_decoder *adsb_create(const adsb_config *cfg_in)
{
    if ((g_cpu_refusal = adsb_host_cpu_refusal()) != nullptr)
        return nullptr;
    adsb_config cfg;
    adsb_debug_config dbg;
    if (const char *why = adsb::accept_config(cfg_in, cfg, dbg)) {
        g_create_error = why;
        return nullptr;
    }
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) {
        g_create_error = std::string("no HIP device available: ") +
                         (e != hipSuccess ? hipGetErrorString(e) : "device count is 0") +
                         " (libadsbdec_amd has no CPU fallback)";
        return nullptr;
    }
    int dev = cfg.device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess)
        dev = 0;
    if (dev >= ndev) {
        g_create_error = "adsb_config.device is out of range";
        return nullptr;
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, dev) != hipSuccess) {
        g_create_error = "hipGetDeviceProperties failed";
        return nullptr;
    }
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        g_create_error = std::string("device is ") + prop.gcnArchName +
                         "; this library carries gfx950 (MI355X) code objects only";
        return nullptr;
    }
    adsb_decoder *d = new (std::nothrow) adsb_decoder();
    if (!d) {
        g_create_error = "out of memory";
        return nullptr;
    }
    d->cfg = cfg;
    d->dbg = dbg;
    d->device = dev;
    d->stage_cap = cfg.stage_samples ? round_down(cfg.stage_samples + 7, 8) : kDefaultStageSamples;
    if (d->stage_cap < (1u << 16))
        d->stage_cap = 1u << 16;

    std::thread warm, warm2; // cfg.warm_start: the process's first-use costs, paid beside the rest of this function
    struct JoinWarm {
        std::thread &a, &b;
        void join()
        {
            if (a.joinable())
                a.join();
            if (b.joinable())
                b.join();
        }
        ~JoinWarm() { join(); }
    } join_warm{warm, warm2}; // (every way out of this function waits for them)
    auto bail = [&](const char *what, hipError_t err) -> adsb_decoder * {
        g_create_error = std::string(what) + ": " + hipGetErrorString(err);
        join_warm.join();
        adsb_destroy(d);
        return nullptr;
    };
    if ((e = hipSetDevice(dev)) != hipSuccess)
        return bail("hipSetDevice", e);
    if (cfg.stream)
        d->stream.adopt(static_cast<hipStream_t>(cfg.stream));
    else if ((e = d->stream.create()) != hipSuccess)
        return bail("hipStreamCreate", e);
    // The staging buffers first, so that a one-shot process (cfg.warm_start: the C host program) can pay the runtime's
    // first-use cost of a large page-locked host-to-device copy -- 7-9 ms inside the first such hipMemcpyAsync of a process,
    // profiles/r5_cli_timing.txt -- on a thread of its own while this one creates the other four streams (5-6 ms each).
    for (int i = 0; i < 2; i++)
        if ((e = d->stage[i].reserve(d->stage_cap)) != hipSuccess)
            return bail("hipMalloc(stage)", e);
    if (cfg.warm_start) {
        const size_t bytes = std::min<size_t>(32u << 20, d->stage_cap * sizeof(uint16_t));
        try {
            warm = std::thread([d, bytes] {
                void *tmp = nullptr;
                if (hipSetDevice(d->device) != hipSuccess || hipHostMalloc(&tmp, bytes, hipHostMallocDefault) != hipSuccess)
                    return; // (best effort: the first push then pays what it always paid)
                std::memset(tmp, 0, 4096);
                // into BOTH staging buffers: the first copy into the second one -- at the stream's first compaction, seven
                // pushes into a 510 MiB file -- cost the C host program another 7 ms (profiles/r6_cli_timing.txt)
                for (int i = 0; i < 2; i++)
                    if (hipMemcpyAsync(d->stage[i], tmp, bytes, hipMemcpyHostToDevice, d->stream) != hipSuccess)
                        break;
                (void)hipStreamSynchronize(d->stream);
                (void)hipHostFree(tmp);
            });
        } catch (...) { // no thread to be had: nothing is warmed
        }
    }
    if (d->stream.owned && !(tuning_env("ADSB_ALT_STREAMS") && atoi(tuning_env("ADSB_ALT_STREAMS")) == 0) &&
        (e = d->stream2.create()) != hipSuccess)
        return bail("hipStreamCreate(second scan stream)", e);
    for (int i = 0; i < adsb_decoder::kCopyStreams; i++)
        if ((e = d->copy_stream[i].create()) != hipSuccess || (e = d->ev_copy[i].create(hipEventDisableTiming)) != hipSuccess)
            return bail("hipStreamCreate(copy)", e);
    if ((e = d->ev_tail.create(hipEventDisableTiming)) != hipSuccess)
        return bail("hipEventCreate(tail)", e);
    if (cfg.warm_start) {
        // ... and the first KERNEL on each copy stream: the staging buffer's first compaction puts the tail's copy kernel on
        // one of them, and the first dispatch on a stream that has only ever carried copies took 7 ms in the middle of the C
        // host program's pushes (profiles/r6_cli_timing.txt: push 7)
        try {
            warm2 = std::thread([d] {
                if (hipSetDevice(d->device) != hipSuccess)
                    return;
                for (hipStream_t cs : d->copy_stream)
                    (void)adsb::launch_copy_samples(d->stage[1] + 64, d->stage[1], 8, cs);
                // ... and the SECOND copy engine.  The runtime asks which engines are idle and takes another one when the
                // usual one is busy (hsa_amd_memory_copy_engine_status, hsa_amd_memory_async_copy_on_engine); an engine's
                // queue is created at its first use, 7.5 ms inside that call -- for the C host program in the copy behind
                // its first compaction, the first one issued while the previous piece's copy was still running
                // (profiles/r6_cli_trace.txt).  Two copies in flight at once, here, beside the rest of adsb_create.
                void *tmp = nullptr;
                const size_t bytes = std::min<size_t>(16u << 20, d->stage_cap * sizeof(uint16_t) / 4);
                if (hipHostMalloc(&tmp, bytes, hipHostMallocDefault) == hipSuccess) {
                    std::memset(tmp, 0, 4096);
                    for (int rep = 0; rep < 2; rep++)
                        for (int i = 0; i < adsb_decoder::kCopyStreams; i++)
                            (void)hipMemcpyAsync(reinterpret_cast<char *>(d->stage[1].p) + (size_t)i * bytes, tmp, bytes, hipMemcpyHostToDevice,
                                                 d->copy_stream[i]);
                }
                for (hipStream_t cs : d->copy_stream)
                    (void)hipStreamSynchronize(cs);
                if (tmp)
                    (void)hipHostFree(tmp);
            });
        } catch (...) {
        }
    }
    for (ScanSlot &sl : d->slots) {
        if ((e = sl.d_counters.reserve(adsb::kDevCounterWords)) != hipSuccess)
            return bail("hipMalloc(counters)", e);
        if ((e = hipMemset(sl.d_counters, 0, adsb::kDevCounterWords * sizeof(uint32_t))) != hipSuccess)
            return bail("hipMemset(counters)", e);
        if ((e = sl.h_counters.reserve(2 * adsb::kCounterWords)) != hipSuccess)
            return bail("hipHostMalloc(counters)", e);
        if ((e = sl.ev_ready[0].create()) != hipSuccess || (e = sl.ev_ready[1].create()) != hipSuccess)
            return bail("hipEventCreate", e);
    }
    {
        std::vector<uint32_t> synd(adsb::kSyndWords);
        adsb::make_syndrome_table(synd.data());
        if ((e = d->d_synd.reserve(synd.size())) != hipSuccess)
            return bail("hipMalloc(synd)", e);
        if ((e = hipMemcpy(d->d_synd, synd.data(), synd.size() * sizeof(uint32_t), hipMemcpyHostToDevice)) != hipSuccess)
            return bail("hipMemcpy(synd)", e);
    }
    if (cfg.fix_1bit) {
        std::vector<uint32_t> fix(adsb::kFixSlots);
        d->fix_mul = adsb::make_fix_table(fix.data());
        if ((e = d->d_fix.reserve(fix.size())) != hipSuccess)
            return bail("hipMalloc(fix)", e);
        if ((e = hipMemcpy(d->d_fix, fix.data(), fix.size() * sizeof(uint32_t), hipMemcpyHostToDevice)) != hipSuccess)
            return bail("hipMemcpy(fix)", e);
    }
    if (cfg.collect_stats) {
        for (int i = 0; i < 2; i++)
            if ((e = d->d_carry[i].reserve(kCarryCap)) != hipSuccess)
                return bail("hipMalloc(try carry)", e);
        // one allocation, so that adsb_reset clears both with one fill: 4 accumulators + 3 (4) carry counts
        if ((e = d->d_try_acc.reserve(kTryStateBytes / sizeof(unsigned long long))) != hipSuccess ||
            (e = hipMemset(d->d_try_acc, 0, kTryStateBytes)) != hipSuccess)
            return bail("hipMalloc(try counters)", e);
        d->d_carry_n = reinterpret_cast<uint32_t *>(d->d_try_acc.p + 4);
        d->frames_cap = 1u << 16; // accepted frames between two count passes (a 128 Mi-offset launch at 1 k frames/s: 13 k)
        if (dbg.frames_cap > 0) // tests: start small, so that the regrow path runs
            d->frames_cap = std::max<size_t>(8, (size_t)dbg.frames_cap);
        for (int i = 0; i < adsb_decoder::kFrameBufs; i++)
            if ((e = d->h_frames[i].reserve(d->frames_cap)) != hipSuccess || (e = d->ev_frames[i].create()) != hipSuccess)
                return bail("hipHostMalloc(accepted frames)", e);
        if ((e = d->d_frames.reserve(d->frames_cap)) != hipSuccess)
            return bail("hipMalloc(accepted frames)", e);
        int prio_least = 0, prio_greatest = 0; // the count passes give way to the scans they run beside
        (void)hipDeviceGetStreamPriorityRange(&prio_least, &prio_greatest);
        if ((e = d->count_stream.create_with_priority(prio_least)) != hipSuccess)
            return bail("hipStreamCreate(count)", e);
        for (ScanSlot &sl : d->slots)
            if ((e = sl.ev_count.create(hipEventDisableTiming)) != hipSuccess)
                return bail("hipEventCreate(count)", e);
        d->res.log_accepted(true);
        d->res.log_into(reinterpret_cast<adsb::Resolver::LogEntry *>(d->h_frames[0] + 1), d->frames_cap - 1);
    }
    d->n_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    {
        if (dbg.reader_min_tiles > 0)
            d->reader_min_tiles = (uint32_t)dbg.reader_min_tiles;
        if (d->cfg.host_threads >= 2)
            start_reader(d);
        if (d->cfg.host_threads >= 3)
            start_gang(d, std::min(d->cfg.host_threads - 2, 15));
    }
    d->no_streaming = dbg.no_streaming != 0;
    if (dbg.shard_head > 0)
        d->shard_head = (uint64_t)dbg.shard_head;
    d->dbg_async = tuning_env("ADSB_DEBUG_ASYNC") ? atoi(tuning_env("ADSB_DEBUG_ASYNC")) : 0;
    d->res.reset();
    join_warm.join();
    return d;
}

// Quiesce, then delete: the reader and the gang are stopped and every stream is waited for BEFORE anything is freed.
void adsb_destroy(adsb_decoder *d)
{
    if (!d)
        return;
    (void)hipSetDevice(d->device);
    if (d->reader) {
        d->reader->stop();
        delete d->reader;
    }
    if (d->gang) {
        d->res.set_gang(nullptr);
        d->gang->stop();
        delete d->gang;
    }
    for (hipStream_t cs : d->copy_stream)
        if (cs)
            (void)wait_stream(d, cs, "a copy stream (adsb_destroy)");
    if (d->stream)
        (void)wait_stream(d, d->stream, "the scan stream (adsb_destroy)");
    if (d->stream2)
        (void)wait_stream(d, d->stream2, "the second scan stream (adsb_destroy)");
    if (d->count_stream)
        (void)wait_stream(d, d->count_stream, "the try-count stream (adsb_destroy)");
    // Nothing on the device can touch the handle's memory any more: its buffers and events free themselves, and its streams
    // behind them (the order of the members in decoder_state.hpp)
    delete d;
}

int adsb_reset(adsb_decoder *d)
{
    if (!d)
        return -1;
    bool busy = d->slot_count != 0;
    for (const ScanSlot &sl : d->slots)
        busy |= sl.busy;
    if (busy) {
        // launches still in flight (a push failed half-way, or adsb_push_async without adsb_sync):
        // let them end before their slots are reused -- their records are dropped with the stream
        HIP_TRY(d, hipSetDevice(d->device));
        for (hipStream_t cs : d->copy_stream)
            WAIT_STREAM(d, cs, "a copy stream");
        WAIT_STREAM(d, d->stream, "the scan stream");
        if (d->stream2)
            WAIT_STREAM(d, d->stream2, "the second scan stream");
        if (d->count_stream) {
            if (count_flush(d))
                return -1;
            WAIT_STREAM(d, d->count_stream, "the try-count stream");
        }
        for (ScanSlot &sl : d->slots) {
            // normally the report kernel behind each scan has left the counters zero; after a failed launch it may not have
            HIP_TRY(d, hipMemsetAsync(sl.d_counters, 0, adsb::kDevCounterWords * sizeof(uint32_t), d->stream));
            sl.launch_stream = nullptr; // every stream has been drained: nothing of the slot's past to order against ...
            sl.busy = false;
            sl.count_pending = false;
            sl.prof_pending[0] = sl.prof_pending[1] = false;
        }
        // ... except these fills: the slot's next launch may go to the second scan stream, which nothing orders behind
        // d->stream -- a late fill would zero the counters of a running scan
        WAIT_STREAM(d, d->stream, "the scan stream");
    }
    else if (wait_last_copy(d)) // a late asynchronous copy must not land in stage[0] beside the next stream's
        return -1;
    if (d->fmt_dirty) { // (every conversion of the stream has ended: a push returns behind its scans, or its copy was just waited for)
        if (format_counters(d, d->fmt_base))
            return -1;
        d->fmt_dirty = false;
    }
    d->fmt_converted = 0;
    d->piece = 0;
    d->shard_on = false;
    d->final_follows = false;
    d->deferred_n = 0;
    d->deferred_slot = nullptr;
    d->deferred_base = 0;
    d->sink = ScanSink{};
    d->n_samples = 0;
    d->kind = adsb::kKindNone;
    d->g_scanned = 0;
    d->seam_offsets = 0;
    d->finished = false;
    d->stage_first = 0;
    d->stage_fill = 0;
    d->cur = 0;
    d->res.reset();
    d->res.log_accepted(d->cfg.collect_stats != 0);
    d->batch_frames.clear(); // (what a batch call handed out is gone with the next reset, like adsb_take's frames)
    d->batch_stats_on = false;
    if (d->acc_dirty) { // behind any count pass still queued -- or still to be enqueued (count_flush)
        if (d->pending.valid) {
            d->pending.clear_after = true;
        } else {
            HIP_TRY(d, hipSetDevice(d->device));
            HIP_TRY(d, hipMemsetAsync(d->d_try_acc, 0, kTryStateBytes, d->count_stream));
        }
    }
    d->acc_dirty = false;
    d->tries_unread = false;
    d->carry_maybe = false;
    d->have_prev_frame = false;
    // In a statistics run slot_head keeps turning: the next stream's first scan then does not have to wait for
    // the count pass that the last launch of this one left behind on the count stream.  Otherwise a stream of
    // one launch stays in slot 0 (the other slots' buffers are never allocated).
    if (!d->cfg.collect_stats)
        d->slot_head = 0;
    d->slot_count = 0;
    d->err.clear();
    return 0;
}

// Follow the reference through the wraps of its sample counter instead of refusing a stream at 2^32 samples.
int adsb_set_long_stream(adsb_decoder *d, int on)
{
    if (!d)
        return -1;
    if (d->n_samples || d->finished || d->slot_count || d->stage_fill || d->shard_on)
        return d->fail("adsb_set_long_stream: only on a fresh or reset handle, before the first push");
    if (on && d->flush)
        return d->fail("adsb_set_long_stream: the handle was given adsb_set_flush, and a long stream has no flush (adsb_set_flush(d, 0) first)");
    if (on && !d->seam_out) {
        HIP_TRY(d, hipSetDevice(d->device));
        HIP_TRY(d, d->seam_out.reserve(adsb::kSeamOutWords));
        HIP_TRY(d, d->seam_slot.ev_ready[0].create(hipEventDisableTiming));
        HIP_TRY(d, d->seam_slot.ev_count.create(hipEventDisableTiming));
    }
    d->long_stream = on != 0;
    return 0;
}

// Decode a stream to its last sample: its end counts as its silent twin's (DESIGN.md "Flush"; resolver.hpp stream_end).
int adsb_set_flush(adsb_decoder *d, int on)
{
    if (!d)
        return -1;
    if (d->n_samples || d->finished || d->slot_count || d->stage_fill || d->shard_on)
        return d->fail("adsb_set_flush: only on a fresh or reset handle, before the first push");
    if (on && d->long_stream)
        return d->fail("adsb_set_flush: the handle was given adsb_set_long_stream, and a long stream has no flush (adsb_set_long_stream(d, 0) first)");
    d->flush = on != 0;
    return 0;
}

int adsb_get_flush(const adsb_decoder *d)
{
    return d ? (d->flush ? 1 : 0) : -1;
}

int adsb_get_wraps(const adsb_decoder *d, uint64_t *wraps, uint64_t *seam_offsets)
{
    if (!d)
        return -1;
    if (wraps)
        *wraps = d->n_samples >> 32; // (the counter has wrapped once the stream holds 2^32 samples)
    if (seam_offsets)
        *seam_offsets = d->seam_offsets;
    return 0;
}

// "0000:c1:00.0" of HIP device `device`, as sysfs spells it (lower case); false: the runtime does not say
static bool device_bdf(int device, char (&bdf)[64])
{
    if (hipDeviceGetPCIBusId(bdf, (int)sizeof bdf, device) != hipSuccess)
        return false;
    for (char *c = bdf; *c; c++)
        if (*c >= 'A' && *c <= 'F')
            *c = (char)(*c - 'A' + 'a');
    return true;
}

int adsb_device_numa_node(int device)
{
    char bdf[64], path[160];
    if (!device_bdf(device, bdf))
        return -1;
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bdf);
    FILE *f = fopen(path, "r");
    int node = -1;
    if (f) {
        if (fscanf(f, "%d", &node) != 1)
            node = -1;
        fclose(f);
    }
    return node;
}

int adsb_device_cpulist(int device, char *out, size_t cap)
{
    if (!out || cap < 2)
        return -1;
    out[0] = 0;
    char bdf[64];
    if (!device_bdf(device, bdf))
        return -1;
    char path[160];
    if (adsb_device_numa_node(device) < 0)
        return 0;
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/local_cpulist", bdf);
    FILE *f = fopen(path, "r");
    if (!f)
        return 0;
    const bool got = fgets(out, (int)cap, f) != nullptr;
    fclose(f);
    if (!got) {
        out[0] = 0;
        return 0;
    }
    size_t n = std::strlen(out);
    while (n && (out[n - 1] == '\n' || out[n - 1] == ' '))
        out[--n] = 0;
    return (int)n;
}

int adsb_host_register(void *p, size_t bytes)
{
    return (p && bytes && hipHostRegister(p, bytes, hipHostRegisterPortable) == hipSuccess) ? 0 : -1;
}

int adsb_host_unregister(void *p)
{
    return (p && hipHostUnregister(p) == hipSuccess) ? 0 : -1;
}

void *adsb_host_alloc(size_t bytes)
{
    void *p = nullptr;
    if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) // (every device of the process may copy from it)
        return nullptr;
    return p;
}

void adsb_host_free(void *p)
{
    if (p && !adsb_host_release_mapped(p)) // (adsb_host_alloc_on / adsb_multi_host_alloc: a mapping of numa.cpp's)
        (void)hipHostFree(p);
}

const char *adsb_last_error(const adsb_decoder *d)
{
    return d ? d->err.c_str() : g_cpu_refusal ? g_cpu_refusal : g_create_error.c_str();
}

} // extern "C"
