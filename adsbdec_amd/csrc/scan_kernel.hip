// scan_kernel.hip -- the fused demodulation kernel for gfx950 (MI355X).
//
// One launch evaluates EVERY preamble offset g in [g_begin, g_end) of a stream of
// real uint16 20 MS/s samples and appends a record for each offset at which the
// reference would have found a CRC-valid frame had it visited that offset:
//
//   air.c:54-92     u16 -> f32, fs/4 sign, 14-tap FIR (7 I + 7 Q), |.|^2, /2 decimation
//   demod.c:102-107 preamble test   p1 > 2*s1 && p2 > 2*s2  (f32 add -> int)
//   demod.c:46-81   DF gate on byte 0 (DF11 / DF17 / DF18 with -a)
//   demod.c:31-44   PPM slicer, 8 strict '>' compares per byte
//   crc.h:36-42     CRC-24 residual == 0 (valid.c:51,73)
//
// The greedy skip, ts and the end-of-file horizon are sequential and are replayed
// on the host over these sparse records (resolver.hpp).
//
// Structure (a streaming integer+f32 scan, VALU-bound on gfx950; no MFMA -- there is no
// contraction, and every product and sum must be rounded separately):
//
//  Stage A (all the arithmetic; no barriers, no divergence).  A thread computes a
//  RUN of 28 consecutive power samples in registers.  28 = 4 x 7 keeps the FIR's
//  summation order -- which in the reference depends on (sample index mod 14), i.e.
//  on m mod 7 -- a compile-time property of each output, so the seven
//  rounding orders are straight-line code with immediate taps.  Every comparison
//  the reference will ever make on those samples is then reduced to ONE BIT per
//  power sample, packed 28 to a word ("bit planes"):
//      D [m] = a[m]   > a[m+5]                (every slicer / DF-gate decision)
//      E1[m] = c[m]   > 2*c[m+5]              (p1 > 2*s1 for the offset g = m)
//      E2[m] = c[m+5] > 2*c[m]                (p2 > 2*s2 for the offset g = m-30)
//  with c[m] = (int)(a[m] + a[m+10]) -- all four preamble sums of demod.c:102-105
//  have that form.  The 16 samples a thread needs from the following run come from
//  the next lane by DPP (wave_shl:1); lane 63 of a wave re-computes the first run
//  of the next wave (1/64 redundancy) so waves never exchange data and Stage A has
//  no barrier.  Power samples never leave registers; LDS receives 12 bytes per 28
//  samples.
//
//  Stage B (bit logic).  For the 28 offsets of a run the preamble test and the DF
//  gate are ~30 word-wide bit operations on funnel-shifted plane words (SIMD within
//  a register: no per-offset branch).  Survivors (~0.5 % of offsets on noise) are
//  compacted through an LDS queue, so the slicer runs with dense lanes.  The slicer
//  gathers the 112 frame bits as 14 columns of 8 bits (bit k = 14b + c sits in word
//  +5b at a fixed bit position, because 140 = 5 x 28) and checks the CRC as the XOR
//  of 14 syndrome-table lookups; only CRC-valid offsets (~1e-4) take the slow path
//  that rebuilds the bytes in order and recomputes pw from the input samples.
//  CRC-valid candidates of the tile are filtered (never-visited rule), ranked, and leave
//  as one write-through store of adjacent lanes into the host's hand-off stream
//  (scan_kernel.h), or -- fallbacks -- through the launch-wide loose list.
//
//  One workgroup of four waves per tile: Stage A, a barrier, Stage B between barriers.  (A pipelined variant -- persistent
//  five-wave workgroups, Stage B of tile t on a wave of its own beside Stage A of tile t + 1 -- was built in round 3,
//  bit-identical and 45 % slower; it and the other experiments that lost are in the history of this file, see
//  DESIGN_HISTORY.md.)
//
//  A workgroup owns owned_runs(K) = 252 K - 44 runs and computes 252 K (+1): the halo
//  (the 1196-sample reach of a long frame) costs 44 runs of planes per tile (2 % at
//  K = 8) instead of 1204 float samples of LDS.
//
// Arithmetic rounds like strict binary32 multiply, then add (built with -ffp-contract=off: the compiler contracts
// nothing).  The fused operations in the ISA are written here, each rounding the real number the reference's separate
// operation rounds: the 56 sign tests of the preamble comparison, the FIR's products on the converted sample and the
// accumulations of its twelve shared products ("The FIR of one run" below); tests/test_build_flags.py counts them.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <type_traits>

#include "power_ordered.h" // taps, power_ordered<>, columns_to_bytes: shared with seam_kernel.hip
#include "scan_kernel.h"
#include "slicer_bits.h"
#include "scan_stamps.h" // ADSB_STAMP / ADSB_COUNT: nothing in the shipped build (a measurement build's per-phase tile clocks)
#include "scan_stages.h" // stage_a, stage_b and what they use
#include "scan_tile.h"   // the tile shell, the stagger, the launcher (after scan_stages.h: see there)

namespace adsb {

// The classic kernel: one workgroup of four waves per tile; Stage A, a barrier, Stage B between barriers (scan_tile.h).
// (Over scan_tile the kernel differs from its own former lines at three sites that run once per tile; timed against them,
// interleaved, inside the run's A/A: profiles/r31_tile_shell_isa_identity.txt, r31_tile_shell_ab.txt.)
template <bool kStats>
__global__ __launch_bounds__(kThreads, kMinWaves) void scan_kernel(const ScanArgs args)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t smem[];
    const int K = tile_passes(blockIdx.x, args.big_tiles, args.passes);
    stagger_start();
    const uint64_t prof_begin = args.profile ? __builtin_amdgcn_s_memrealtime() : 0; // (the launch's duration: scan_tile's last lines)
    const int64_t t0 = // first owned offset
        (int64_t)args.g_begin + (int64_t)kRun * (int64_t)tile_first_run(blockIdx.x, args.big_tiles, args.passes);
    scan_tile<kStats, kFrontReal>(args, K, t0, prof_begin, smem);
}

// Behind every scan launch, one wave: hand the launch counters to the host (two
// write-through granules into pinned memory) and leave them zero for the slot's next
// launch.  This replaces a runtime copy kernel, a fill kernel and the gap between them
// (measured: 16 us per launch of a multi-launch stream, against ~4 us).  Letting the last
// tile to finish do it instead -- a `done` counter -- was measured too: every tile then waits
// for its atomics to return before it can retire, and the kernel ran 25 % slower.
__global__ __launch_bounds__(64) void report_kernel(uint32_t *counters, uint32_t *report, uint32_t gen)
{
    if (threadIdx.x != 0)
        return;
    unsigned long long *c64 = reinterpret_cast<unsigned long long *>(counters);
    const uint32_t c0 = atomicExch(&counters[0], 0u), c1 = atomicExch(&counters[1 * kCounterPad], 0u),
                   c2 = atomicExch(&counters[2 * kCounterPad], 0u);
    atomicExch(&counters[3 * kCounterPad], 0u);
    const unsigned long long nb = atomicExch(&c64[2 * kCounterPad], 0ull), en = atomicExch(&c64[(5 * kCounterPad) / 2], 0ull);
    store_granule_through(report, 0, u32x4{c0, c1, c2, gen});
    store_granule_through(report, 1, u32x4{(uint32_t)nb, (uint32_t)(nb >> 32), (uint32_t)en, (uint32_t)(en >> 32)});
}

// Is g inside an accepted frame that starts before it?  (The frame's own offset is a visited Try: strict
// inequality.)  Binary search over the whole frame array: the list and carry entries, and tiles whose window
// of frames does not fit a wave.
__device__ __forceinline__ bool try_shadowed(const TryCountArgs &a, uint64_t g)
{
    uint32_t lo = 0, hi = a.n_frames;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (a.frames[mid].g < g)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo > 0 && g < a.frames[lo - 1].g + a.frames[lo - 1].span;
}

// Blocks [0, ceil(n_tiles / 4)): one WAVE per tile region.  The accepted frames that can shadow a try of the
// tile start inside (t0 - 1200, t0 + tile offsets): the wave finds the first of them with a 64-way search (three
// rounds of one load per lane for 13 k frames, instead of 14 dependent loads per try), keeps the window one
// frame per lane, and tests every try against it on lane broadcasts.  Measured: the per-try binary search took
// 34 us per 256 Mi samples with 8 192 resident waves, and slowed the scan kernel running beside it by as much.
// The remaining blocks: the launch-wide list and the carry of earlier passes, grid-stride.
constexpr int kCountThreads = 256;
// Blocks that walk the tile regions, four tiles at a time each (grid-stride).  The pass runs beside the NEXT launch's scan, which
// is bound by VALU issue: with one block per four tiles (697 for a 256 Mi-sample launch) that scan took 0.156 ms, with 256 or 64
// blocks 0.149 ms and the statistics step 2 % less; with 16 the pass itself (0.33 ms) became the step, and with 64 a stream of
// eight launches (2 Gi samples) ended 0.3 ms later, its passes queued up behind the scans (profiles/r4_ab_runs.txt section 8).
constexpr int kCountRegionGrid = 256;
// (32 VGPRs: what five resident scan waves of 96 leave free on a SIMD of 512.  Round 6's first version of the four-words-per-lane
// loop took 40 and no longer fitted beside the scan it runs next to: the pass took 72 us instead of 53 on the sparse capture and
// the scan beside it 3 % longer -- profiles/r6_ab_runs.txt section 5.)
__global__ __launch_bounds__(kCountThreads) void count_tries_kernel(const TryCountArgs a)
{
    uint32_t cnt[3] = {0, 0, 0};
    const uint32_t region_blocks = a.regions ? (a.n_tiles + 3u) / 4u : 0u;
    auto carry = [&](uint64_t g, uint32_t code) { // the scan has not got there yet
        if (a.final)
            return;
        const uint32_t slot = atomicAdd(a.n_carry_out, 1u);
        if (slot < a.carry_cap)
            a.carry_out[slot] = (g << 2) | code;
        else
            a.acc[3] = 1; // reported when the statistics are read
    };
    const uint32_t region_grid = min(region_blocks, (uint32_t)kCountRegionGrid);
    if (blockIdx.x < region_grid) {
      for (uint32_t rb = blockIdx.x; rb < region_blocks; rb += region_grid) {
        const uint32_t tile = rb * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
        const uint32_t n = tile < a.n_tiles ? min(a.region_counts[tile], (uint32_t)kTryRegion) : 0u;
        if (n) { // wave-uniform
            const uint64_t t0 = a.g_base + (uint64_t)kRun * tile_first_run(tile, a.big_tiles, a.passes);
            const uint64_t t1 = t0 + (uint64_t)kRun * (uint64_t)owned_runs(tile_passes(tile, a.big_tiles, a.passes));
            const uint64_t key = t0 >= (uint64_t)(ADSB_DECOFFSET_K - 1) ? t0 - (ADSB_DECOFFSET_K - 1) : 0; // frames below cannot reach t0
            // first frame with g >= key: the answer lies in [lo, hi]
            uint32_t lo = 0, hi = a.n_frames;
            while (lo < hi) {
                const uint32_t step = (hi - lo + 63u) / 64u, idx = lo + lane * step;
                const bool below = idx < hi && a.frames[idx].g < key; // true for a prefix of the lanes
                const uint32_t k = (uint32_t)__popcll(__ballot(below));
                if (k == 0) {
                    hi = lo;
                } else {
                    const uint32_t nlo = lo + (k - 1u) * step + 1u;
                    hi = min(lo + k * step, hi);
                    lo = nlo;
                }
            }
            // the window, one frame per lane, relative to key (everything fits 32 bits)
            const uint32_t fi = lo + lane;
            const bool have = fi < a.n_frames && a.frames[fi].g < t1;
            const uint32_t fr = have ? (uint32_t)(a.frames[fi].g - key) : 0xFFFFFFFFu;
            const uint32_t fe = have ? fr + a.frames[fi].span : 0u;
            const uint32_t w = (uint32_t)__popcll(__ballot(have));
            const bool fits = w < 64u || lo + 64u >= a.n_frames || a.frames[lo + 64u].g >= t1; // wave-uniform
            const uint32_t *reg = a.regions + (size_t)tile * kTryRegion;
            const uint32_t base_minus_key = (uint32_t)(a.g_base - key); // (mod 2^32: key may lie up to 1199 offsets below the launch's base)
            const uint32_t hi_rel = a.hi <= a.g_base ? 0u : (uint32_t)std::min<uint64_t>(a.hi - a.g_base, 0xFFFFFFFFull); // tries at or beyond are carried
            // kW tries per lane and round: the loads are in flight together (a region of the adversarial capture holds 3 600
            // words: one load per round and lane was 57 dependent round trips per tile), and a broadcast of the window serves kW
            // comparisons.  kW = 2, not 4: the pass has to fit the 32 registers that five resident scan waves leave free on a SIMD
            // (with 4 it took 40, ran 72 us instead of 53 on the sparse capture and cost the scan beside it 3 %).
            constexpr int kW = 2;
            for (uint32_t i0 = 0; i0 < n; i0 += 64u * kW) {
                uint32_t word[kW];
                bool live[kW];
#pragma unroll
                for (int u = 0; u < kW; u++) {
                    const uint32_t i = i0 + 64u * (uint32_t)u + lane;
                    live[u] = i < n;
                    word[u] = live[u] ? reg[i] : 0u;
                }
                // (32-bit arithmetic relative to the launch's base and to the window's key: the pass has 32 registers)
                uint32_t rt[kW];
                bool shadowed[kW] = {};
#pragma unroll
                for (int u = 0; u < kW; u++) {
                    const uint32_t gr = word[u] >> 2;
                    rt[u] = gr + base_minus_key; // (only looked at for tries below a.hi: those lie inside the tile)
                    if (live[u] && gr >= hi_rel) {
                        carry(a.g_base + gr, word[u] & 3u);
                        live[u] = false;
                    }
                }
                if (fits) {
                    for (uint32_t j = 0; j < w; j++) { // (w is wave-uniform)
                        const uint32_t fj = __builtin_amdgcn_readlane(fr, j), ej = __builtin_amdgcn_readlane(fe, j);
#pragma unroll
                        for (int u = 0; u < kW; u++)
                            shadowed[u] |= fj < rt[u] && rt[u] < ej;
                    }
                } else {
#pragma unroll
                    for (int u = 0; u < kW; u++)
                        shadowed[u] = live[u] && try_shadowed(a, a.g_base + (word[u] >> 2));
                }
#pragma unroll
                for (int u = 0; u < kW; u++)
                    if (live[u] && !shadowed[u]) {
                        const uint32_t code = word[u] & 3u;
                        cnt[code < 3 ? code : 2]++;
                    }
            }
        }
      }
    } else {
        const uint32_t n_carry = min(*a.n_carry, a.carry_cap);
        if (blockIdx.x == region_grid && threadIdx.x == 0)
            *a.n_carry_next = 0; // three counts in rotation: nobody reads or appends to this one during this pass
        const uint32_t total = a.n_tries + n_carry;
        const uint32_t nb = gridDim.x - region_grid;
        for (uint32_t i = (blockIdx.x - region_grid) * blockDim.x + threadIdx.x; i < total; i += nb * blockDim.x) {
            uint64_t g;
            uint32_t code;
            if (i < a.n_tries) {
                const uint32_t w = a.tries[i];
                g = a.g_base + (w >> 2);
                code = w & 3u;
            } else {
                const uint64_t w = a.carry_in[i - a.n_tries];
                g = w >> 2;
                code = (uint32_t)w & 3u;
            }
            if (g >= a.hi) {
                carry(g, code);
                continue;
            }
            if (!try_shadowed(a, g))
                cnt[code < 3 ? code : 2]++;
        }
    }
    // one atomic per block and counter: same-address atomics serialise in L2
    __shared__ uint32_t part[3];
    if (threadIdx.x < 3)
        part[threadIdx.x] = 0;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 3; k++) {
        uint32_t v = cnt[k];
        for (int off = 32; off > 0; off >>= 1)
            v += __shfl_down(v, off);
        if ((threadIdx.x & 63) == 0 && v)
            atomicAdd(&part[k], v);
    }
    __syncthreads();
    if (threadIdx.x < 3 && part[threadIdx.x])
        atomicAdd(&a.acc[threadIdx.x], (unsigned long long)part[threadIdx.x]);
}

hipError_t launch_count_tries(const TryCountArgs &args, hipStream_t stream)
{
    // the carry count lives on the device: a fixed number of blocks, grid-stride over whatever there is
    const uint32_t region_blocks = args.regions ? (args.n_tiles + 3u) / 4u : 0u;
    const uint32_t guess = args.n_tries + 65536u;
    // (beside the tile regions the list is what did not fit them -- rare, short -- and the carry: 64 blocks, so that the pass stays
    // small beside the next scan; a LONG list -- a launch forced onto it, tiles beyond 4 096 passes -- is a latency-bound chain
    // of look-ups per thread and needs the threads: one block per 2 048 words, up to 1 024)
    const uint32_t cap = args.regions ? std::min<uint32_t>(1024u, std::max<uint32_t>(64u, args.n_tries / 2048u)) : 2048u;
    const unsigned list_blocks = (unsigned)std::min<uint32_t>((guess + kCountThreads - 1u) / kCountThreads, cap);
    const uint32_t region_grid = std::min<uint32_t>(region_blocks, (uint32_t)kCountRegionGrid);
    hipLaunchKernelGGL(count_tries_kernel, dim3(region_grid + list_blocks), dim3(kCountThreads), 0, stream, args);
    return hipGetLastError();
}

void make_syndrome_table(uint32_t *out)
{
    // S[k] = x^(111-k) mod G, G = x^24 + 0xFFF409 (crc.h): the residual of
    // valid.c:49-51,71-73 is the XOR of S[k] over the set frame bits k.
    uint32_t s[112];
    uint32_t r = 1;
    for (int e = 0; e < 112; e++) {
        s[111 - e] = r;
        r <<= 1;
        if (r & 0x1000000u)
            r ^= 0x1FFF409u;
    }
    for (int c = 0; c < 14; c++)
        for (int v = 0; v < 256; v++) {
            uint32_t acc = 0;
            for (int b = 0; b < 8; b++)
                if (v & (1 << b))
                    acc ^= s[14 * b + c];
            out[c * 256 + v] = acc;
        }
}

uint32_t make_fix_table(uint32_t *tab)
{
    uint32_t syn[112];
    uint32_t r = 1;
    for (int e = 0; e < 112; e++) {
        syn[111 - e] = r;
        r <<= 1;
        if (r & 0x1000000u)
            r ^= 0x1FFF409u;
    }
    for (uint32_t mul = 0x9E3779B1u;; mul += 2) {
        for (int i = 0; i < kFixSlots; i++)
            tab[i] = 0;
        bool ok = true;
        for (int k = 5; k < 112 && ok; k++) {
            uint32_t &slot = tab[(uint32_t)(syn[k] * mul) >> 23];
            ok = slot == 0;
            slot = (syn[k] << 8) | (uint32_t)k;
        }
        if (ok)
            return mul;
    }
}

int choose_passes(uint64_t n_offsets, int cus, bool dense)
{
    if (cus <= 0)
        cus = 256;
    // Measured, not modelled (round 6: launches of every size interleaved in one process, K = 2..7 side by side on the
    // kernel's own clock: tools/ab_interleaved.py, profiles/r6_ab_passes_sizes.txt; rounds 1-5 chose by a cost model of
    // "rounds of resident workgroups" that the same measurement refutes -- a large launch's time is 10.7 us + 46 ns per tile,
    // no steps -- and that was up to 14 % off the best K at 16 Mi offsets).  Below ~64 Mi offsets the best K is not monotonic:
    // the launch is one or two device-fulls of tiles and the fill of the last one decides.
    //   offsets (Mi)      1     2     4     8     16    24    32    48    64    80    88   128
    //   best K            2     2     3     3     5     5     3     3     4     6     6     7
    //   next best, +%   3:17  3:13  2:7   2:4   2:10  4:5   7:2   5:2   5:1   7:2   5:2   6:1
    // From K = 8 on a CU's LDS holds four workgroups, not five (+7 % and more).  At 128 Mi offsets, K = 4 / 5 / 6 / 7 / 8:
    // sparse 1.045 / 1.036 / 1.007 / 1 / 1.067, noise the same; BASELINE configs[2] at its stated density 0.970 / 0.981 /
    // 0.972 / 1 / 1.093, with the Try/Ok table 0.961 / 0.939 / 0.938 / 1: a tile of frames back to back stages fewer
    // candidates for its all-pairs filter and overflows its survivor queue less often.  `dense` = the handle's previous
    // launch handed over a record per 2 048 offsets or more.
    const uint64_t n = n_offsets * 256u / (uint64_t)cus; // (the table is a 256-CU device's)
    constexpr struct {
        uint32_t below_mi;
        int k;
    } table[] = {{3, 2}, {12, 3}, {28, 5}, {56, 3}, {72, 4}, {96, 6}};
    for (const auto &row : table)
        if (n < ((uint64_t)row.below_mi << 20))
            return row.k;
    return dense ? 6 : 7;
}

// The staging buffer's unscanned tail (a few KB) moved to the other buffer, by a kernel of the library's own: the
// runtime's device-to-device copy loads its blit kernels on first use -- 7 ms inside the first such hipMemcpyAsync of a
// process, a quarter of what the C host program needs to decode a 510 MiB capture (profiles/r5_cli_timing.txt).  src and dst are
// 16-byte aligned (the tail starts on a 128-byte line of one buffer and goes to the first sample of the other).
__global__ __launch_bounds__(256) void copy_samples_kernel(uint16_t *__restrict__ dst, const uint16_t *__restrict__ src, size_t n)
{
    const size_t n8 = n / 8, stride = (size_t)gridDim.x * blockDim.x;
    const u32x4 *s4 = reinterpret_cast<const u32x4 *>(src);
    u32x4 *d4 = reinterpret_cast<u32x4 *>(dst);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride)
        d4[i] = s4[i];
    if (blockIdx.x == 0 && threadIdx.x < n - 8 * n8)
        dst[8 * n8 + threadIdx.x] = src[8 * n8 + threadIdx.x];
}

hipError_t launch_copy_samples(uint16_t *dst, const uint16_t *src, size_t n, hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    if ((reinterpret_cast<uintptr_t>(dst) | reinterpret_cast<uintptr_t>(src)) & 15u) // (not the tail's case: let the runtime do it)
        return hipMemcpyAsync(dst, src, n * sizeof(uint16_t), hipMemcpyDeviceToDevice, stream);
    const unsigned blocks = (unsigned)std::min<size_t>(1024, (n / 8 + 255) / 256 + 1);
    hipLaunchKernelGGL(copy_samples_kernel, dim3(blocks), dim3(256), 0, stream, dst, src, n);
    return hipGetLastError();
}

hipError_t launch_report(const ScanArgs &args, hipStream_t stream)
{
    if (args.report)
        hipLaunchKernelGGL(report_kernel, dim3(1), dim3(64), 0, stream, args.counters, args.report, args.gen);
    return hipGetLastError();
}

hipError_t launch_scan(const ScanArgs &args, bool stats, hipStream_t stream)
{
    return launch_stream_tiles(scan_kernel<true>, scan_kernel<false>, args, stats, stream);
}

} // namespace adsb
