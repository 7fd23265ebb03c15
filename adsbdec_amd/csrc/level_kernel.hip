// level_kernel.hip -- the level report of a capture's power samples (include/adsbdec_amd.h: the adsb_level_* calls): a histogram of
// their bit patterns in 2048 bins (bits >> 20: 8 bins per octave), the maximum of every run of 28 (the envelope), the samples with
// the sign bit set, and the input's codes on its rails.  Every quantity is a count or an unsigned maximum, so any order of
// reduction gives the same bits (adsbdec_amd/levels.py level_report is the definition).
//
// level_kernel is power_export_kernel (power_export_kernel.hip) up to the end of its FIR: the same pass structure (a wave covers
// 64 runs of 28 power samples, grid-stride) and the same front end -- scan_stages.h real_front, the one definition of the typed
// loads, the plain-load road, the constants and the FIR that stage_a and the exports call too (profiles/r24_front_shared_isa.txt:
// each compiles to the instructions it had with lines of its own) -- and then, instead of the export's stores, the reduction tail.
// level_units_kernel is the same tail behind an element-wise front end: a lane takes 28 complex int16 samples, complex int8
// samples or float32 power samples (seven 16-byte loads where the array is 16-byte aligned, as scan_power_kernel's; unit by unit
// where it is not, and in the capture's last run).
//
// The tail, per lane and pass: the run's 28 bit patterns -> one unsigned maximum (a float per lane, 256 contiguous bytes per wave);
// 28 increments of a histogram in LDS; the codes the lane OWNS -> the rail counters.  A lane's window overlaps its neighbour's by
// six pairs: the counters look at slots 6 .. 33 only.  Counters are counted per wave on the scalar side: a compare into a lane mask,
// its population count, a scalar add.
//
// Accumulation (DESIGN.md section 4 "Level report" has the measurements; ADSB_LEVEL_HIST picks in a measurement build, the
// shipped one defines nothing).  The build runs with the compiler's atomic optimizer off, so an LDS add is one per lane; 32-bit
// counts cannot overflow (a capture has fewer than 2^32 power samples).
//   bit 0: 0 one histogram per workgroup (8 KiB), 1 one per wave (32 KiB)
//   bit 1: the wave-uniform shortcut -- when every counting lane of an increment hits the same bin, ONE lane adds their number.
//          Silence puts all 64 x 28 increments of a pass on bin 0.
//   bit 2: the run-uniform shortcut instead -- a lane whose 28 samples fall in one bin adds their number at once.  It costs a
//          minimum beside the envelope's maximum and one compare per run, where bit 1 costs two lane masks per increment.
// Shipped: 5, a histogram per wave with the run-uniform shortcut.
// The flush (ADSB_LEVEL_FLUSH): 0 the workgroup adds its non-zero bins to the 64-bit totals with vector atomics, eight
// wave-instructions of 512 contiguous bytes; 1 it writes a row of 32-bit counts and level_reduce_kernel sums the rows.
// ADSB_LEVEL_BLOCKS caps the grid: fewer workgroups, fewer adds on the same words.
#include "scan_stages.h"

#include <algorithm>

#include "level.h"
#include "level_tail.h" // Counts, level_tail, rails_real, rails_iq, unit_bits: shared with level_batch_kernel.hip

#ifndef ADSB_LEVEL_FLUSH
#define ADSB_LEVEL_FLUSH 0
#endif
#ifndef ADSB_LEVEL_BLOCKS
#define ADSB_LEVEL_BLOCKS 2048
#endif

namespace adsb {

namespace {

constexpr int kHistCopies = (ADSB_LEVEL_HIST & 1) ? kWaves : 1;
constexpr int kRowsSlices = 16;       // level_reduce_kernel: the rows are summed in this many interleaved slices

// ---- what a workgroup does before its first pass and behind its last ----
__device__ __forceinline__ void block_begin(uint32_t (*hist)[kLevelBins], uint32_t *cnt)
{
    uint32_t *flat = &hist[0][0];
    for (int i = threadIdx.x; i < kHistCopies * kLevelBins; i += kThreads)
        flat[i] = 0;
    if (threadIdx.x < 4)
        cnt[threadIdx.x] = 0;
    __syncthreads();
}

__device__ __forceinline__ void block_end(uint32_t (*hist)[kLevelBins], uint32_t *cnt, const Counts &c, const int lane,
                                          unsigned long long *__restrict__ totals, uint32_t *__restrict__ rows)
{
    if (lane == 0) { // the waves' counters meet in LDS: one add per workgroup and counter leaves it
        if (c.negative)
            atomicAdd(&cnt[0], c.negative);
        if (c.rail_lo)
            atomicAdd(&cnt[1], c.rail_lo);
        if (c.rail_hi)
            atomicAdd(&cnt[2], c.rail_hi);
        if (c.over)
            atomicAdd(&cnt[3], c.over);
    }
    __syncthreads();
#if ADSB_LEVEL_FLUSH == 1
    uint32_t *row = rows + (size_t)blockIdx.x * kLevelRowWords;
    if (threadIdx.x < 4)
        row[threadIdx.x] = cnt[threadIdx.x];
#else
    if (threadIdx.x < 4 && cnt[threadIdx.x])
        atomicAdd(&totals[1 + threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
#endif
#pragma unroll
    for (int j = 0; j < kLevelBins / kThreads; j++) {
        const int bin = j * kThreads + threadIdx.x;
        uint32_t v = 0;
#pragma unroll
        for (int w = 0; w < kHistCopies; w++)
            v += hist[w][bin];
#if ADSB_LEVEL_FLUSH == 1
        row[4 + bin] = v;
#else
        if (v)
            atomicAdd(&totals[5 + bin], (unsigned long long)v);
#endif
    }
}

__global__ __launch_bounds__(kThreads) void level_kernel(const uint32_t *__restrict__ xin, const int64_t p_hi, const int64_t m_end,
                                                         unsigned long long *__restrict__ totals, float *__restrict__ env,
                                                         uint32_t *__restrict__ rows)
{
    __shared__ uint32_t hist[kHistCopies][kLevelBins];
    __shared__ uint32_t cnt[4];
    const int lane = threadIdx.x & 63;
    const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t *my_hist = hist[(ADSB_LEVEL_HIST & 1) ? wave_in_block : 0];
    block_begin(hist, cnt);
    Counts c;
    const int64_t n_passes = (m_end + kWavePass - 1) / kWavePass; // a pass: one wave, 64 runs
    const int64_t stride = (int64_t)gridDim.x * kWaves;
#pragma unroll 1
    for (int64_t pass = (int64_t)blockIdx.x * kWaves + wave_in_block; pass < n_passes; pass += stride) {
        const int64_t w0 = pass * kWavePass; // the wave's first power sample = lane 0's first pair: a multiple of 28
        f32x2 vv[34];
        float a[kRun];
        real_front<false>(xin, 0, 0, p_hi, w0 - 8, lane, vv, a); // (the wave's window starts 8 pairs below)

        // the lane's run is power samples [m0, m0 + 28), of which those below m_end exist; the lane owns their pairs, slots 6 .. 33
        const int64_t m0 = w0 + (int64_t)kRun * lane;
        const int left = (int)std::min<int64_t>(kRun, std::max<int64_t>(0, m_end - m0));
        const bool full = w0 + kWavePass <= m_end; // (wave-uniform)
        uint32_t b[kRun];
#pragma unroll
        for (int k = 0; k < kRun; k++)
            b[k] = __builtin_bit_cast(uint32_t, a[k]);
        // (a sum of two squares of finite floats: the sign bit is never set)
        const uint32_t mx = full ? level_tail<true, false>(b, kRun, my_hist, c, lane) : level_tail<false, false>(b, left, my_hist, c, lane);
        if (full)
            rails_real<true>(vv, kRun, c);
        else
            rails_real<false>(vv, left, c);
        if (env && left > 0)
            env[pass * 64 + lane] = __builtin_bit_cast(float, mx);
    }
    block_end(hist, cnt, c, lane, totals, rows);
}

template <int kKind>
__global__ __launch_bounds__(kThreads) void level_units_kernel(const void *__restrict__ xin, const size_t n, unsigned long long *__restrict__ totals,
                                                               float *__restrict__ env, uint32_t *__restrict__ rows)
{
    __shared__ uint32_t hist[kHistCopies][kLevelBins];
    __shared__ uint32_t cnt[4];
    const int lane = threadIdx.x & 63;
    const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint32_t *my_hist = hist[(ADSB_LEVEL_HIST & 1) ? wave_in_block : 0];
    block_begin(hist, cnt);
    Counts c;
    const size_t n_passes = (n + kWavePass - 1) / kWavePass;
    const size_t stride = (size_t)gridDim.x * kWaves;
    constexpr size_t kUnit = kKind == kLevelIq8 ? 2 : 4;
    const bool aligned = (uintptr_t)xin % (4 * kUnit) == 0; // (a run is 28 units: every lane's is then aligned as the array is)
#pragma unroll 1
    for (size_t pass = (size_t)blockIdx.x * kWaves + wave_in_block; pass < n_passes; pass += stride) {
        const size_t w0 = pass * kWavePass, m0 = w0 + (size_t)kRun * lane;
        const bool full = w0 + kWavePass <= n; // (wave-uniform)
        const int left = m0 >= n ? 0 : (int)std::min<size_t>(kRun, n - m0);
        uint32_t u[kRun];
        if (full && aligned) {
            if constexpr (kKind == kLevelIq8) {
                const u32x2 *p = reinterpret_cast<const u32x2 *>(static_cast<const uint16_t *>(xin) + m0);
#pragma unroll
                for (int k = 0; k < kRun / 4; k++) {
                    const u32x2 q = p[k];
                    u[4 * k] = q.x & 0xFFFFu, u[4 * k + 1] = q.x >> 16, u[4 * k + 2] = q.y & 0xFFFFu, u[4 * k + 3] = q.y >> 16;
                }
            } else {
                const u32x4 *p = reinterpret_cast<const u32x4 *>(static_cast<const uint32_t *>(xin) + m0);
#pragma unroll
                for (int k = 0; k < kRun / 4; k++) {
                    const u32x4 q = p[k];
                    u[4 * k] = q.x, u[4 * k + 1] = q.y, u[4 * k + 2] = q.z, u[4 * k + 3] = q.w;
                }
            }
        } else {
#pragma unroll
            for (int k = 0; k < kRun; k++) {
                u[k] = 0;
                if (k < left)
                    u[k] = kKind == kLevelIq8 ? (uint32_t) static_cast<const uint16_t *>(xin)[m0 + k] : static_cast<const uint32_t *>(xin)[m0 + k];
            }
        }
        uint32_t b[kRun];
#pragma unroll
        for (int k = 0; k < kRun; k++)
            b[k] = unit_bits<kKind>(u[k]);
        constexpr bool kSigned = kKind == kLevelPower;
        const uint32_t mx = full ? level_tail<true, kSigned>(b, kRun, my_hist, c, lane) : level_tail<false, kSigned>(b, left, my_hist, c, lane);
        if constexpr (kKind != kLevelPower) {
            if (full)
                rails_iq<kKind, true>(u, kRun, c);
            else
                rails_iq<kKind, false>(u, left, c);
        }
        if (env && left > 0)
            env[pass * 64 + lane] = __builtin_bit_cast(float, mx);
    }
    block_end(hist, cnt, c, lane, totals, rows);
}

// ADSB_LEVEL_FLUSH == 1: column `col` of the rows of `blocks` workgroups, every kRowsSlices-th from blockIdx.y on, added to the totals
__global__ __launch_bounds__(256) void level_reduce_kernel(const uint32_t *__restrict__ rows, const unsigned blocks,
                                                           unsigned long long *__restrict__ totals)
{
    const unsigned col = blockIdx.x * 256 + threadIdx.x;
    if (col >= (unsigned)kLevelRowWords)
        return;
    unsigned long long v = 0;
    for (unsigned r = blockIdx.y; r < blocks; r += kRowsSlices)
        v += rows[(size_t)r * kLevelRowWords + col];
    if (v)
        atomicAdd(&totals[1 + col], v);
}

hipError_t reduce_rows(const uint32_t *rows, unsigned blocks, unsigned long long *totals, hipStream_t stream)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || !level_uses_rows())
        return e;
    hipLaunchKernelGGL(level_reduce_kernel, dim3((kLevelRowWords + 255) / 256, kRowsSlices), dim3(256), 0, stream, rows, blocks, totals);
    return hipGetLastError();
}

} // namespace

unsigned level_max_blocks() { return ADSB_LEVEL_BLOCKS; }
bool level_uses_rows() { return ADSB_LEVEL_FLUSH == 1; }

hipError_t launch_level(const uint32_t *x, int64_t p_hi, int64_t m_end, unsigned long long *totals, float *env, uint32_t *rows,
                        hipStream_t stream)
{
    if (m_end <= 0)
        return hipSuccess;
    const uint64_t passes = ((uint64_t)m_end + kWavePass - 1) / kWavePass;
    const unsigned blocks = (unsigned)std::min<uint64_t>(level_max_blocks(), (passes + kWaves - 1) / kWaves);
    hipLaunchKernelGGL(level_kernel, dim3(blocks), dim3(kThreads), 0, stream, x, p_hi, m_end, totals, env, rows);
    return reduce_rows(rows, blocks, totals, stream);
}

hipError_t launch_level_units(int kind, const void *x, size_t n, unsigned long long *totals, float *env, uint32_t *rows, hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    const uint64_t passes = ((uint64_t)n + kWavePass - 1) / kWavePass;
    const unsigned blocks = (unsigned)std::min<uint64_t>(level_max_blocks(), (passes + kWaves - 1) / kWaves);
    if (kind == kLevelIq16)
        hipLaunchKernelGGL(level_units_kernel<kLevelIq16>, dim3(blocks), dim3(kThreads), 0, stream, x, n, totals, env, rows);
    else if (kind == kLevelIq8)
        hipLaunchKernelGGL(level_units_kernel<kLevelIq8>, dim3(blocks), dim3(kThreads), 0, stream, x, n, totals, env, rows);
    else
        hipLaunchKernelGGL(level_units_kernel<kLevelPower>, dim3(blocks), dim3(kThreads), 0, stream, x, n, totals, env, rows);
    return reduce_rows(rows, blocks, totals, stream);
}

} // namespace adsb
