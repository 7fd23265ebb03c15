// power_export_batch_kernel.hip -- the power samples of a BATCH of captures, written out by ONE launch (include/adsbdec_amd.h: the
// adsb_power_batch_* calls; decoder_export_batch.hip).
//
// power_export_batch_kernel is power_export_kernel (power_export_kernel.hip) with the capture looked up per pass.  The passes of
// all captures are numbered in one space (power_export_batch.hpp); a wave's pass number is wave-uniform, so the row it lies in is
// found once per pass by scalar loads and wave-uniform compares -- the way unpack12_batch.hip finds a chunk's rows -- and no lane
// ever searches.  With the row in hand the body is power_export_kernel's with pbuf0 = p_lo = 0, m_begin = 0 and the row's p_hi,
// m_end, x and out: every capture is a fresh stream of its own, whose six pairs in front of pair 0 read as silence whatever lies
// in front of it in memory.  The same 17 typed buffer loads where the wave's window is interior, the same plain-load road at a
// capture's start and ragged end, the same power_run<0>, the same 7 KiB-per-wave LDS turn for whole waves, the same seven 16-byte
// stores for a ragged last wave and float-by-float stores for the last run.  The FIRST pass of every capture takes the plain-load
// road (its window starts 8 pairs below pair 0): 1 pass in 293 of a 1 Mi-sample capture, every pass of a capture below 3584
// samples (DESIGN.md section 4 "Batch export").
// The load block is a copy of power_export_kernel's, which is a copy of stage_a's, for the reason given there: a function shared
// with them moved the existing units' code, and those units compile to the instructions they had.
// The table is read through the constant address space: nothing writes it while the kernel runs, and said so, its wave-uniform
// reads stay scalar loads behind the load block's memory clobber and the kernel's own stores.  The addresses read from it are
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

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) ExportSeg *const_table;
typedef const __attribute__((address_space(1))) uint32_t *global_words;
typedef __attribute__((address_space(1))) float *global_floats;
typedef __attribute__((address_space(1))) f32x4 *global_f32x4;

constexpr int kExportWave = 64 * kRun; // power samples of a wave's pass
static_assert((uint64_t)kExportWave == kExportPass, "power_export_batch.hpp restates the pass of scan_kernel.h's run");

__global__ __launch_bounds__(kThreads) void power_export_batch_kernel(const ExportSeg *__restrict__ tab_in, const uint32_t n_rows,
                                                                      const uint64_t n_passes)
{
    __shared__ f32x4 turn[kWaves][kExportWave / 4];
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
        // the FIR's constants, written per pass as stage_a writes them (fir_product)
        FirConsts kc = {{{0, 0}, {0, 0}, {0, 0}, {0, 0}}, {{tap<12>(), tap<13>()}, {tap<10>(), tap<11>()}, {tap<8>(), tap<9>()}, {tap<6>(), tap<7>()}}};
#define ADSB_KC(b, T0, T1)                                                                                                          \
    asm volatile("v_mov_b32 %0, %2\n\tv_mov_b32 %1, %3"                                                                            \
                 : "=v"(kc.c2048[b].x), "=v"(kc.c2048[b].y)                                                                         \
                 : "i"(__builtin_bit_cast(uint32_t, 2048.0f * tap<T0>())), "i"(__builtin_bit_cast(uint32_t, 2048.0f * tap<T1>())))
        ADSB_KC(0, 12, 13);
        ADSB_KC(1, 10, 11);
        ADSB_KC(2, 8, 9);
        ADSB_KC(3, 6, 7);
#undef ADSB_KC
#pragma unroll
        for (int b = 0; b < 4; b++)
            asm volatile("" : "+s"(kc.taps[b]));
        const int64_t w0 = pass * kExportWave; // the wave's first power sample = lane 0's first pair: a multiple of 28
        const int64_t wlo = w0 - 8;            // lane 0's window starts 8 pairs below (two of them are never read)
        // wave-uniform: every pair this wave loads lies inside the capture (never in its first pass)
        const bool interior = (wlo >= 0) && (wlo + kRun * 64 + 8 <= p_hi);
        f32x4 tl[17]; // tl[k]: pairs 2k+2, 2k+3 of the lane's 36 = slots 2k, 2k+1
        if (interior) {
            const uint64_t wbase = (uint64_t)(xin + wlo);
            i32x4 rs;
            rs.x = __builtin_amdgcn_readfirstlane((int)(uint32_t)wbase);
            rs.y = __builtin_amdgcn_readfirstlane((int)((uint32_t)(wbase >> 32) & 0xFFFFu)); // stride 0: raw buffer
            rs.z = 64 * kRun * 4 + 64;                                                        // bytes
            rs.w = (int)(4u | 5u << 3 | 6u << 6 | 7u << 9 /* dst_sel xyzw */ | 2u << 12 /* USCALED */ | 12u << 15 /* 16_16_16_16 */);
            const int voff = lane * (kRun * 4);
            // (s_nop 4: should a descriptor word reach its register through a v_readfirstlane, the first load is five states behind it)
            asm volatile("s_nop 4\n\t"
                         "buffer_load_format_xyzw %0, %17, %18, 0 offen offset:8\n\t"
                         "buffer_load_format_xyzw %1, %17, %18, 0 offen offset:16\n\t"
                         "buffer_load_format_xyzw %2, %17, %18, 0 offen offset:24\n\t"
                         "buffer_load_format_xyzw %3, %17, %18, 0 offen offset:32\n\t"
                         "buffer_load_format_xyzw %4, %17, %18, 0 offen offset:40\n\t"
                         "buffer_load_format_xyzw %5, %17, %18, 0 offen offset:48\n\t"
                         "buffer_load_format_xyzw %6, %17, %18, 0 offen offset:56\n\t"
                         "buffer_load_format_xyzw %7, %17, %18, 0 offen offset:64\n\t"
                         "buffer_load_format_xyzw %8, %17, %18, 0 offen offset:72\n\t"
                         "buffer_load_format_xyzw %9, %17, %18, 0 offen offset:80\n\t"
                         "buffer_load_format_xyzw %10, %17, %18, 0 offen offset:88\n\t"
                         "buffer_load_format_xyzw %11, %17, %18, 0 offen offset:96\n\t"
                         "buffer_load_format_xyzw %12, %17, %18, 0 offen offset:104\n\t"
                         "buffer_load_format_xyzw %13, %17, %18, 0 offen offset:112\n\t"
                         "buffer_load_format_xyzw %14, %17, %18, 0 offen offset:120\n\t"
                         "buffer_load_format_xyzw %15, %17, %18, 0 offen offset:128\n\t"
                         "buffer_load_format_xyzw %16, %17, %18, 0 offen offset:136"
                         "\n\ts_waitcnt vmcnt(0)"
                         : "=&v"(tl[0]), "=&v"(tl[1]), "=&v"(tl[2]), "=&v"(tl[3]), "=&v"(tl[4]), "=&v"(tl[5]), "=&v"(tl[6]),
                           "=&v"(tl[7]), "=&v"(tl[8]), "=&v"(tl[9]), "=&v"(tl[10]), "=&v"(tl[11]), "=&v"(tl[12]),
                           "=&v"(tl[13]), "=&v"(tl[14]), "=&v"(tl[15]), "=&v"(tl[16])
                         : "v"(voff), "s"(rs)
                         : "memory");
        } else {
            // The capture's start -- a stream's start: the reference's zero-initialised ring (air.c:33: a missing pair is
            // 0x0800,0x0800 -> v = 0), never the neighbouring capture's samples -- and its ragged end: plain loads, converted here
            int64_t pr0 = wlo + (int64_t)kRun * lane;
            asm volatile("" : "+v"(pr0)); // (opaque, as in stage_a: the 34 pair indices of this rare path are not precomputed and spilled)
#pragma unroll
            for (int k = 0; k < 17; k++) {
                const int64_t pa = pr0 + 2 * k + 2, pb = pa + 1;
                const uint32_t d0 = (pa >= 0 && pa < p_hi) ? xin[pa] : 0x08000800u;
                const uint32_t d1 = (pb >= 0 && pb < p_hi) ? xin[pb] : 0x08000800u;
                tl[k] = f32x4{(float)(d0 & 0xFFFFu), (float)(d0 >> 16), (float)(d1 & 0xFFFFu), (float)(d1 >> 16)};
            }
        }
        // the run's pairs as (I, Q), slot s <-> pair s - 6 of the run (the - 2048 and the fs/4 sign are inside the FIR's products)
        f32x2 vv[34];
#pragma unroll
        for (int s = 0; s < 34; s++) {
            const f32x4 q = tl[s >> 1];
            vv[s] = (s & 1) ? f32x2{q.z, q.w} : f32x2{q.x, q.y};
        }
        float a[kRun];
        power_run<0>(vv, a, kc);

        // the lane's run is power samples [m0, m0 + 28) of the capture, which ends at m_end, anywhere
        const int64_t m0 = w0 + (int64_t)kRun * lane;
        const global_floats o = out + m0; // 112 bytes per lane: 16-byte aligned
        if (w0 + kExportWave <= m_end) { // (wave-uniform) a whole wave: lane L's 16-byte piece j <-> piece 7 L + j of the wave's 448
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
