// power_export_kernel.hip -- the front end's power samples, written out (include/adsbdec_amd.h: the adsb_power_* calls).
//
// power_export_kernel is Stage A of the scan (scan_stages.h stage_a) up to the end of its FIR and no further: the same 17 typed
// buffer loads of a lane's 34 pairs over the wave's window, the same plain-load road where the window leaves the buffer, the same
// constants written per pass, the same power_run<0> -- and then the 28 floats of the run go to memory instead of into sign planes.
// No planes, no Stage B, no workgroup barrier.  What differs from stage_a:
//   * all 64 lanes of a wave own a run (no lane that only feeds its neighbour): a wave covers 64 x 28 = 1792 power samples;
//   * the indices are the stream's: a run starts at a multiple of 28 power samples of the STREAM, so the output's phase
//     (m mod 7) and the pair's fs/4 sign (m mod 2) are the compile-time properties of the slot that the FIR takes them for;
//   * a lane's 28 floats are 112 contiguous bytes at out[m - m_begin].  A wave whose 1792 samples all lie inside the window turns
//     them through 7 KiB of LDS of its own (seven 16-byte writes at the lane's 112 bytes, seven 16-byte reads at piece 64 k + lane:
//     wave-private, so no barrier beyond the wave's own), and every store instruction then writes 1 KiB of contiguous lines.  The
//     window's last, ragged wave stores each lane's own 112 bytes as seven 16-byte stores, and its last run float by float.
//     Measured (profiles/r17_power_export.txt, DESIGN.md section 4 "Power export"): seven 16-byte stores per lane, 112 bytes apart
//     by lane as the loads are, take 1.29 x the time of the transposed layout and 4.4 x when non-temporal; non-temporal stores of
//     the transposed layout's full lines make no difference (1.008, the run's A/A 1.011), so the plain ones ship.
//     ADSB_EXPORT_STORE picks the layout in a measurement build (tools/format_probe.py --export --layout); the shipped one defines nothing.
// The load block is a copy of stage_a's: a function shared with it moved the existing units' code (DESIGN.md section 4 "IQ
// captures"), and those units compile to the instructions they had.
//
// iq_power_export_kernel: a[m] = iq_power(complex sample m) -- two rounded products, one rounded sum, nothing fused: 16 bytes
// in, 16 bytes out per lane, grid-stride.
#include "scan_stages.h"

#include <algorithm>

#include "power_export.h"

#ifndef ADSB_EXPORT_STORE
#define ADSB_EXPORT_STORE 2 // 2: a whole wave's samples transposed through LDS; 0: seven plain 16-byte stores per lane; 1, 3: as 0, 2 with non-temporal stores
#endif

namespace adsb {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int kExportWave = 64 * kRun; // power samples of a wave's pass

__device__ __forceinline__ void store16(f32x4 *p, f32x4 v)
{
#if ADSB_EXPORT_STORE & 1
    __builtin_nontemporal_store(v, p);
#else
    *p = v;
#endif
}

__global__ __launch_bounds__(kThreads) void power_export_kernel(const uint32_t *__restrict__ xin, const int64_t pbuf0, const int64_t p_lo,
                                                                const int64_t p_hi, const int64_t m_begin, const int64_t m_end,
                                                                float *__restrict__ out)
{
#if ADSB_EXPORT_STORE >= 2
    __shared__ f32x4 turn[kWaves][kExportWave / 4];
#endif
    const int lane = threadIdx.x & 63;
    const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t n_passes = (m_end - m_begin + kExportWave - 1) / kExportWave; // a pass: one wave, 64 runs
    const int64_t stride = (int64_t)gridDim.x * kWaves;
#pragma unroll 1
    for (int64_t pass = (int64_t)blockIdx.x * kWaves + wave_in_block; pass < n_passes; pass += stride) {
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
        const int64_t w0 = m_begin + pass * kExportWave; // the wave's first power sample = lane 0's first pair: a multiple of 28
        const int64_t wlo = w0 - 8;                      // lane 0's window starts 8 pairs below (two of them are never read)
        // wave-uniform: every pair this wave loads lies inside the buffer
        const bool interior = (wlo >= p_lo) && (wlo + kRun * 64 + 8 <= p_hi);
        f32x4 tl[17]; // tl[k]: pairs 2k+2, 2k+3 of the lane's 36 = slots 2k, 2k+1
        if (interior) {
            const uint64_t wbase = (uint64_t)(xin + (wlo - pbuf0));
            i32x4 rs;
            rs.x = __builtin_amdgcn_readfirstlane((int)(uint32_t)wbase);
            rs.y = __builtin_amdgcn_readfirstlane((int)((uint32_t)(wbase >> 32) & 0xFFFFu)); // stride 0: raw buffer
            rs.z = 64 * kRun * 4 + 64;                                                        // bytes
            rs.w = (int)(4u | 5u << 3 | 6u << 6 | 7u << 9 /* dst_sel xyzw */ | 2u << 12 /* USCALED */ | 12u << 15 /* 16_16_16_16 */);
            const int voff = lane * (kRun * 4);
            asm volatile("buffer_load_format_xyzw %0, %17, %18, 0 offen offset:8\n\t"
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
            // The start of the buffer -- at the stream's start the reference's zero-initialised ring (air.c:33: a missing pair is
            // 0x0800,0x0800 -> v = 0), elsewhere the caller's choice (adsbdec_amd.h: the window rule) -- and its ragged end:
            // plain loads, converted here
            int64_t pr0 = wlo + (int64_t)kRun * lane;
            asm volatile("" : "+v"(pr0)); // (opaque, as in stage_a: the 34 pair indices of this rare path are not precomputed and spilled)
#pragma unroll
            for (int k = 0; k < 17; k++) {
                const int64_t pa = pr0 + 2 * k + 2, pb = pa + 1;
                const uint32_t d0 = (pa >= p_lo && pa < p_hi) ? xin[pa - pbuf0] : 0x08000800u;
                const uint32_t d1 = (pb >= p_lo && pb < p_hi) ? xin[pb - pbuf0] : 0x08000800u;
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

        // the lane's run is power samples [m0, m0 + 28); the window ends at m_end, anywhere
        const int64_t m0 = w0 + (int64_t)kRun * lane;
        float *o = out + (m0 - m_begin); // 112 bytes per lane: 16-byte aligned
#if ADSB_EXPORT_STORE >= 2
        if (w0 + kExportWave <= m_end) { // (wave-uniform) a whole wave: lane L's 16-byte piece j <-> piece 7 L + j of the wave's 448
            f32x4 *t = turn[wave_in_block];
#pragma unroll
            for (int k = 0; k < kRun / 4; k++)
                t[(kRun / 4) * lane + k] = f32x4{a[4 * k], a[4 * k + 1], a[4 * k + 2], a[4 * k + 3]};
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            f32x4 *ow = reinterpret_cast<f32x4 *>(out + (w0 - m_begin));
#pragma unroll
            for (int k = 0; k < kRun / 4; k++)
                store16(ow + 64 * k + lane, t[64 * k + lane]); // one instruction: 1 KiB of contiguous lines
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            continue;
        }
#endif
        if (m0 + kRun <= m_end) {
#pragma unroll
            for (int k = 0; k < kRun / 4; k++)
                store16(reinterpret_cast<f32x4 *>(o) + k, f32x4{a[4 * k], a[4 * k + 1], a[4 * k + 2], a[4 * k + 3]});
        } else if (m0 < m_end) { // the window's last run: never past m_end
            const int left = (int)(m_end - m0);
#pragma unroll
            for (int k = 0; k < kRun; k++)
                if (k < left)
                    o[k] = a[k];
        }
    }
}

// 4 complex samples at p (aligned to the 4-byte sample, no more) -> their four power samples
__device__ __forceinline__ f32x4 iq_power4(const uint32_t *p)
{
    uint32_t e[4];
    __builtin_memcpy(e, p, sizeof e);
    return f32x4{iq_power(e[0]), iq_power(e[1]), iq_power(e[2]), iq_power(e[3])};
}

__global__ __launch_bounds__(256) void iq_power_export_kernel(const uint32_t *__restrict__ x, const size_t n, float *__restrict__ out)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x, t = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t groups = n / 4, tail_at = 4 * groups;
    if (tail_at + t < n) // (up to 3 samples: the first lanes of the grid)
        out[tail_at + t] = iq_power(x[tail_at + t]);
    f32x4 *o4 = reinterpret_cast<f32x4 *>(out);
    for (size_t i = t; i < groups; i += stride)
        o4[i] = iq_power4(x + 4 * i); // (plain in every build: ADSB_EXPORT_STORE is power_export_kernel's alone)
}

} // namespace

hipError_t launch_power_export(const uint32_t *x, int64_t pbuf0, int64_t p_lo, int64_t p_hi, int64_t m_begin, int64_t m_end, float *out,
                               hipStream_t stream)
{
    if (m_end <= m_begin)
        return hipSuccess;
    const uint64_t passes = ((uint64_t)(m_end - m_begin) + kExportWave - 1) / kExportWave;
    // as launch_convert: 8 blocks of 256 lanes per CU at most (2048 on the 256 CUs of an MI355X) stream HBM
    const unsigned blocks = (unsigned)std::min<uint64_t>(2048, (passes + kWaves - 1) / kWaves);
    hipLaunchKernelGGL(power_export_kernel, dim3(blocks), dim3(kThreads), 0, stream, x, pbuf0, p_lo, p_hi, m_begin, m_end, out);
    return hipGetLastError();
}

hipError_t launch_iq_power_export(const uint32_t *x, size_t n, float *out, hipStream_t stream)
{
    if (n == 0)
        return hipSuccess;
    const unsigned blocks = (unsigned)std::min<uint64_t>(2048, std::max<uint64_t>(1, (n / 4 + 255) / 256));
    hipLaunchKernelGGL(iq_power_export_kernel, dim3(blocks), dim3(256), 0, stream, x, n, out);
    return hipGetLastError();
}

} // namespace adsb
