// power_export_kernel.hip -- the front end's power samples, written out (include/adsbdec_amd.h: the adsb_power_* calls).
//
// power_export_kernel is Stage A of the scan (scan_stages.h stage_a) up to the end of its FIR and no further: stage_a's front end
// (scan_stages.h real_front: the 17 typed buffer loads of a lane's 34 pairs over the wave's window, the plain-load road where the
// window leaves the buffer, the constants written per pass, power_run<0>) -- and then the 28 floats of the run go to memory instead
// of into sign planes.
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
// The front end is not a copy: real_front (scan_stages.h) is the one definition stage_a, this kernel, the batch export and the
// level report call, and each compiles to the instructions it had with lines of its own (profiles/r24_front_shared_isa.txt).
// The three-way store behind it is still written here and in power_export_batch_kernel.hip: the two spell their addresses
// differently and compile differently, and one text moved the instructions of one or the other (the same record).
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
    __shared__ f32x4 turn[kWaves][kWavePass / 4];
#endif
    const int lane = threadIdx.x & 63;
    const int wave_in_block = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t n_passes = (m_end - m_begin + kWavePass - 1) / kWavePass; // a pass: one wave, 64 runs
    const int64_t stride = (int64_t)gridDim.x * kWaves;
#pragma unroll 1
    for (int64_t pass = (int64_t)blockIdx.x * kWaves + wave_in_block; pass < n_passes; pass += stride) {
        const int64_t w0 = m_begin + pass * kWavePass; // the wave's first power sample = lane 0's first pair: a multiple of 28
        f32x2 vv[34];
        float a[kRun];
        real_front<false>(xin, pbuf0, p_lo, p_hi, w0 - 8, lane, vv, a); // (the wave's window starts 8 pairs below)

        // the lane's run is power samples [m0, m0 + 28); the window ends at m_end, anywhere
        const int64_t m0 = w0 + (int64_t)kRun * lane;
        float *o = out + (m0 - m_begin); // 112 bytes per lane: 16-byte aligned
#if ADSB_EXPORT_STORE >= 2
        if (w0 + kWavePass <= m_end) { // (wave-uniform) a whole wave: lane L's 16-byte piece j <-> piece 7 L + j of the wave's 448
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
    const uint64_t passes = ((uint64_t)(m_end - m_begin) + kWavePass - 1) / kWavePass;
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
