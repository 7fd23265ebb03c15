// power_export_batch_kernel.hip -- the power samples of a BATCH of captures, written out by ONE launch (include/adsbdec_amd.h: the
// adsb_power_batch_* calls; decoder_export_batch.hip).
//
// power_export_batch_kernel is power_export_kernel (power_export_kernel.hip) with the capture looked up per pass.  The passes of
// all captures are numbered in one space (power_export_batch.hpp); a wave's pass number is wave-uniform, so the row it lies in is
// found once per pass by scalar loads and wave-uniform compares -- the way unpack12_batch.hip finds a chunk's rows -- and no lane
// ever searches.  With the row in hand the body is power_export_kernel's with pbuf0 = p_lo = 0, m_begin = 0 and the row's p_hi,
// m_end, x and out: every capture is a fresh stream of its own, whose six pairs in front of pair 0 read as silence whatever lies
// in front of it in memory.  The same front end (scan_stages.h real_front, here with s_nop 4 in front of its typed loads: not a
// copy, and the kernel compiles to the instructions it had with lines of its own, profiles/r24_front_shared_isa.txt), the same
// 7 KiB-per-wave LDS turn for whole waves, the same seven 16-byte stores for a ragged last wave and float-by-float stores for the
// last run (written out here as there: the same record has why).  The FIRST pass of every capture takes the front end's
// plain-load road (its window starts 8 pairs below pair 0): 1 pass in 293 of a 1 Mi-sample capture, every pass of a capture below
// 3584 samples (DESIGN.md section 4 "Batch export").
// The table is read through the constant address space: nothing writes it while the kernel runs, and said so, its wave-uniform
// reads stay scalar loads behind the front end's memory clobber and the kernel's own stores.  The addresses read from it are
// generic ones to the compiler: said to be global memory, as unpack12_batch.hip says it.
//
// iq_power_export_batch_kernel: the same table over groups of four complex samples.  A block takes chunks of 256 groups,
// grid-stride, and looks the rows of a chunk's first and last group up as unpack12_batch_kernel does; a capture's last group
// stores only the samples it has.
#include "scan_stages.h"

#include <algorithm>

#include "power_export_batch.hpp"

namespace adsb {

namespace {

typedef const __attribute__((address_space(4))) ExportSeg *const_table;
typedef const __attribute__((address_space(1))) uint32_t *global_words;
typedef __attribute__((address_space(1))) float *global_floats;
typedef __attribute__((address_space(1))) f32x4 *global_f32x4;

static_assert((uint64_t)kWavePass == kExportPass, "power_export_batch.hpp restates the pass of scan_kernel.h's run");

__global__ __launch_bounds__(kThreads) void power_export_batch_kernel(const ExportSeg *__restrict__ tab_in, const uint32_t n_rows,
                                                                      const uint64_t n_passes)
{
    __shared__ f32x4 turn[kWaves][kWavePass / 4];
    const const_table tab = (const_table)(uintptr_t)tab_in;
    const int lane = threadIdx.x & 63;
    const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint64_t stride = (uint64_t)gridDim.x * kWaves;
#pragma unroll 1
    for (uint64_t unit = (uint64_t)blockIdx.x * kWaves + wave_in_block; unit < n_passes; unit += stride) {
        // the capture this pass belongs to, and the pass's number inside it (wave-uniform: the scalar unit's)
        const uint32_t r = export_row(tab, 0, n_rows - 1, unit);
        const int64_t pass = (int64_t)(unit - tab[r].first);
        const int64_t p_hi = (int64_t)tab[r].p_hi, m_end = (int64_t)tab[r].m_end;
        const global_words xin = (global_words)tab[r].src;
        const global_floats out = (global_floats)tab[r].out;
        const int64_t w0 = pass * kWavePass; // the wave's first power sample = lane 0's first pair: a multiple of 28
        f32x2 vv[34];
        float a[kRun];
        real_front<true>(xin, 0, 0, p_hi, w0 - 8, lane, vv, a); // (the wave's window starts 8 pairs below: never interior in a capture's first pass)

        // the lane's run is power samples [m0, m0 + 28) of the capture, which ends at m_end, anywhere
        const int64_t m0 = w0 + (int64_t)kRun * lane;
        const global_floats o = out + m0; // 112 bytes per lane: 16-byte aligned
        if (w0 + kWavePass <= m_end) { // (wave-uniform) a whole wave: lane L's 16-byte piece j <-> piece 7 L + j of the wave's 448
            f32x4 *t = turn[wave_in_block];
#pragma unroll
            for (int k = 0; k < kRun / 4; k++)
                t[(kRun / 4) * lane + k] = f32x4{a[4 * k], a[4 * k + 1], a[4 * k + 2], a[4 * k + 3]};
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            const global_f32x4 ow = (global_f32x4)(out + w0);
#pragma unroll
            for (int k = 0; k < kRun / 4; k++)
                ow[64 * k + lane] = t[64 * k + lane]; // one instruction: 1 KiB of contiguous lines
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            continue;
        }
        if (m0 + kRun <= m_end) {
#pragma unroll
            for (int k = 0; k < kRun / 4; k++)
                ((global_f32x4)o)[k] = f32x4{a[4 * k], a[4 * k + 1], a[4 * k + 2], a[4 * k + 3]};
        } else if (m0 < m_end) { // the capture's last run: never past m_end
            const int left = (int)(m_end - m0);
#pragma unroll
            for (int k = 0; k < kRun; k++)
                if (k < left)
                    o[k] = a[k];
        }
    }
}

__global__ __launch_bounds__(kExportIqChunk) void iq_power_export_batch_kernel(const ExportSeg *__restrict__ tab_in, const uint32_t n_rows,
                                                                               const uint64_t groups)
{
    const const_table tab = (const_table)(uintptr_t)tab_in;
    const uint64_t chunks = (groups + kExportIqChunk - 1) / kExportIqChunk;
    for (uint64_t c = blockIdx.x; c < chunks; c += gridDim.x) {
        const uint64_t g0 = c * kExportIqChunk, g1 = g0 + (kExportIqChunk - 1) < groups ? g0 + (kExportIqChunk - 1) : groups - 1;
        const uint32_t r0 = export_row(tab, 0, n_rows - 1, g0); // block-uniform: the scalar unit's
        const uint32_t r1 = export_row(tab, r0, n_rows - 1, g1);
        const uint64_t g = g0 + threadIdx.x;
        if (g > g1)
            continue;
        const uint32_t r = export_row(tab, r0, r1, g); // (r0 == r1: no iteration)
        const uint64_t at = kExportIqGroup * (g - tab[r].first), n = tab[r].m_end; // the group's first sample inside its capture
        const global_words x = (global_words)tab[r].src + at; // (aligned to the 4-byte sample, no more)
        const global_floats o = (global_floats)tab[r].out + at;
        if (at + kExportIqGroup <= n) {
            uint32_t e[4];
#pragma unroll
            for (int k = 0; k < 4; k++)
                e[k] = x[k];
            *(global_f32x4)o = f32x4{iq_power(e[0]), iq_power(e[1]), iq_power(e[2]), iq_power(e[3])};
        } else { // the capture's last group: the samples it has
            const int left = (int)(n - at);
#pragma unroll
            for (int k = 0; k < 3; k++)
                if (k < left)
                    o[k] = iq_power(x[k]);
        }
    }
}

} // namespace

hipError_t launch_power_export_batch(const ExportSeg *tab_device, uint32_t n_rows, uint64_t units, hipStream_t stream)
{
    if (units == 0 || n_rows == 0)
        return hipSuccess;
    // as launch_power_export: 8 blocks of 256 lanes per CU at most (2048 on the 256 CUs of an MI355X) stream HBM
    const unsigned blocks = (unsigned)std::min<uint64_t>(2048, (units + kWaves - 1) / kWaves);
    hipLaunchKernelGGL(power_export_batch_kernel, dim3(blocks), dim3(kThreads), 0, stream, tab_device, n_rows, units);
    return hipGetLastError();
}

hipError_t launch_iq_power_export_batch(const ExportSeg *tab_device, uint32_t n_rows, uint64_t units, hipStream_t stream)
{
    if (units == 0 || n_rows == 0)
        return hipSuccess;
    const unsigned blocks = (unsigned)std::min<uint64_t>(2048, (units + kExportIqChunk - 1) / kExportIqChunk);
    hipLaunchKernelGGL(iq_power_export_batch_kernel, dim3(blocks), dim3(kExportIqChunk), 0, stream, tab_device, n_rows, units);
    return hipGetLastError();
}

} // namespace adsb
