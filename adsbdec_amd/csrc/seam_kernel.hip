// seam_kernel.hip -- the offsets around a wrap of the reference's sample counter, for gfx950.
//
// The reference's `fidx` is a uint32_t that counts input samples (air.c:34).  Write a power index as g = w * 2^31 + r: inside
// epoch w the ring phase is that of a fresh stream in r (air.c:65-70 see fidx = 2 r), which is what the scan kernel computes
// when a launch is given epoch-relative indices.  At P = w * 2^31 the counter wraps, 2^32 mod 14 = 4, and the ring is NOT
// cleared: pair q sits in slot pair (q mod 2^31) mod 7 whichever epoch wrote it, and the output behind pair m reads
// `o = 14 - fidx % 14` from the counter as it stands after the pair, c = ((m + 1) mod 2^31) mod 7.  So power samples
// P - 1 .. P + 5 follow neither epoch's formula; every other sample follows its own epoch's, bit for bit.
//
// One workgroup per wrap.  It computes the ~2 400 power samples the seam offsets [P - 1196, P + 28) read into LDS, each by
// its own rule -- power_ordered<p> (power_ordered.h, shared with the scan kernel's pw_at) with p = r mod 7 of the sample's
// OWN epoch, the seven transient samples by the ring rule: slot pair i = 0 .. 6 in order, holding the latest pair q <= m of
// that slot, against taps T[(2 i - 2 c) mod 14], T[.. + 1] (air.c:69-76,84-91: every product rounded, then every sum; the
// build has -ffp-contract=off and this file writes no fused form) -- then the D plane (a[m] > a[m + 5], 28 bits a word, as
// the scan kernel lays it out), and per offset the preamble test (demod.c:102-107), the DF gate (demod.c:46-81), the slicer
// (slicer_bits.h gather_columns), the CRC by the syndrome table and, with fix_tab, the 1-bit repair, as stage_b does.
// Every CRC-valid offset is reported; the host resolver decides (resolver.hpp), in offset order between the records of the
// two launches on either side.  Plain vector stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "power_ordered.h"
#include "scan_kernel.h" // kCandWords, kSyndWords
#include "seam_kernel.h"
#include "slicer_bits.h"

namespace adsb {

namespace {

constexpr int kSeamThreads = 256;
constexpr int kSeamPower = kSeamMaxOffsets + kSeamWindow;      // power samples a launch may need
constexpr int kSeamWords = (kSeamMaxOffsets + 27) / 28 + 44 + 4; // D-plane words gather_columns may read (44 ahead of a run)

template <int K>
__device__ __forceinline__ void fill_taps(float *t)
{
    if constexpr (K < 14) {
        t[K] = tap<K>();
        fill_taps<K + 1>(t);
    }
}

// (x - 2048) of pair q with the fs/4 sign of its index (air.c:64-67,79-82), silence where the buffer has no such pair
__device__ __forceinline__ f32x2 pair_value(const SeamArgs &a, int64_t q)
{
    const uint32_t d = (q >= a.p_lo && q < a.p_hi) ? a.x[q - a.pbuf0] : 0x08000800u;
    const f32x2 f = {(float)(d & 0xFFFFu), (float)(d >> 16)};
    const f32x2 mid = {2048.0f, 2048.0f};
    return ((q & 1) == 0) ? (f - mid) : (mid - f);
}

__device__ __forceinline__ int slot_of(int64_t q) { return (int)((uint32_t)((uint64_t)q & (kEpoch - 1)) % 7u); }

// A sample inside an epoch: the fresh-stream rule in r (pairs m-6 .. m, order p, p-1, .., 0, 6, .., p+1 with p = r mod 7)
__device__ __forceinline__ float power_in_epoch(const SeamArgs &a, int64_t m)
{
    const f32x2 taps[7] = {{tap<12>(), tap<13>()}, {tap<10>(), tap<11>()}, {tap<8>(), tap<9>()}, {tap<6>(), tap<7>()},
                           {tap<4>(), tap<5>()},   {tap<2>(), tap<3>()},   {tap<0>(), tap<1>()}};
    f32x2 pr[7];
#pragma unroll
    for (int age = 0; age < 7; age++)
        pr[age] = taps[age] * pair_value(a, m - age);
    return power_by_phase(pr, slot_of(m));
}

// P - 1 .. P + 5: the ring as the wrapped counter finds it
__device__ __forceinline__ float power_transient(const SeamArgs &a, int64_t m, const float *lt)
{
    const int c = slot_of(m + 1);
    f32x2 s = {0.0f, 0.0f};
#pragma unroll 1
    for (int i = 0; i < 7; i++) {
        int64_t q = m;
#pragma unroll 1
        for (int d = 0; d < 14 && slot_of(q) != i; d++)
            q--;
        const int t = (2 * i - 2 * c + 14) % 14;
        const f32x2 tp = {lt[t], lt[t + 1]};
        const f32x2 pr = tp * pair_value(a, q);
        s = i == 0 ? pr : s + pr; // (0.0f + x == x up to the sign of zero, which the square erases)
    }
    const f32x2 sq = s * s;
    return sq.x + sq.y;
}

__global__ __launch_bounds__(kSeamThreads) void seam_kernel(const SeamArgs a)
{
    __shared__ float pw[kSeamPower + 8];
    __shared__ uint32_t pl_d[kSeamWords];
    __shared__ float lt[16];
    __shared__ uint32_t n_out[2];
    const int tid = (int)threadIdx.x;
    const int64_t base = (int64_t)a.g_begin, P = (int64_t)a.boundary;
    const int n_off = (int)(a.g_end - a.g_begin);      // <= kSeamMaxOffsets (launch_seam checks)
    const int n_pow = n_off - 1 + kSeamWindow;         // <= kSeamPower
    if (tid == 0) {
        fill_taps<0>(lt);
        lt[14] = lt[15] = 0.0f;
        n_out[0] = n_out[1] = 0;
    }
    __syncthreads();
    for (int i = tid; i < n_pow; i += kSeamThreads) {
        const int64_t m = base + i;
        pw[i] = (m >= P - 1 && m <= P + 5) ? power_transient(a, m, lt) : power_in_epoch(a, m);
    }
    __syncthreads();
    if (a.power_out) // (each lane the samples it computed)
        for (int i = tid; i < n_pow; i += kSeamThreads)
            a.power_out[i] = pw[i];
    for (int v = tid; v < kSeamWords; v += kSeamThreads) {
        uint32_t w = 0;
        for (int j = 0; j < 28; j++) {
            const int i = 28 * v + j;
            if (i + 5 < n_pow && pw[i] > pw[i + 5]) // demod.c:38: strict '>'
                w |= 1u << j;
        }
        pl_d[v] = w;
    }
    __syncthreads();
    uint32_t *recs = a.out + kSeamOutHeader, *tries = recs + (size_t)kCandWords * kSeamMaxOffsets;
    for (int rel = tid; rel < n_off; rel += kSeamThreads) {
        // demod.c:102-107: float add, conversion to int by truncation, SN 2
        const int p1 = __float2int_rz(pw[rel] + pw[rel + 10]), s1 = __float2int_rz(pw[rel + 5] + pw[rel + 15]);
        const int p2 = __float2int_rz(pw[rel + 35] + pw[rel + 45]), s2 = __float2int_rz(pw[rel + 30] + pw[rel + 40]);
        if (!(p1 > 2 * s1 && p2 > 2 * s2))
            continue;
        auto dbit = [&](int i) { return (pl_d[i / 28] >> (i % 28)) & 1u; };
        const uint32_t df = dbit(rel + 80) << 4 | dbit(rel + 90) << 3 | dbit(rel + 100) << 2 | dbit(rel + 110) << 1 | dbit(rel + 120);
        uint32_t code; // demod.c:46-81: 01011 (DF11), 10001 (DF17) and, with -a, 10010 (DF18)
        if (df == 11u)
            code = 0;
        else if (df == 17u)
            code = 1;
        else if (df == 18u && a.df18)
            code = 2;
        else
            continue;
        if (a.want_tries) // valid.c:46,68: a Try, if the greedy scan visits it (the count pass decides)
            tries[atomicAdd(&n_out[1], 1u)] = ((uint32_t)rel << 2) | code;
        const int sv = rel / 28, sj = rel % 28;
        uint32_t cw[4];
        gather_columns(pl_d + sv, sj, cw);
        uint32_t syn = 0; // (as stage_b: a short frame's syndromes are the long frame's four rows further on)
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t iw = (code == 0) ? ((cw[j] & 0x0F0F0F0Fu) << 4) : cw[j];
#pragma unroll
            for (int k = 0; k < 4 && 4 * j + k < 14; k++)
                syn ^= a.synd[(4 * j + k) * 256 + ((iw >> (8 * k)) & 0xFFu)];
        }
        uint32_t fixed = 0;
        if (syn != 0) {
            if (!a.fix_tab || code == 0)
                continue;
            const uint32_t e = a.fix_tab[(syn * a.fix_mul) >> 23];
            if ((e >> 8) != syn)
                continue;
            const uint32_t k = e & 0xFFu, kc = k % 14u, kb = k / 14u;
#pragma unroll
            for (int wq = 0; wq < 4; wq++)
                cw[wq] ^= ((kc >> 2) == (uint32_t)wq) ? (1u << (8 * (kc & 3u) + kb)) : 0u;
            fixed = 1;
        }
        uint32_t wds[4];
        columns_to_bytes(cw, code == 0, wds);
        wds[3] |= fixed << 24;
        uint32_t *rec = recs + (size_t)kCandWords * atomicAdd(&n_out[0], 1u); // (one record per offset at most: it fits)
        rec[0] = (uint32_t)rel;
        rec[1] = (uint32_t)((p1 + p2) / 4); // demod.c:127,133
        rec[2] = wds[0];
        rec[3] = wds[1];
        rec[4] = wds[2];
        rec[5] = wds[3];
    }
    __syncthreads();
    if (tid == 0) {
        a.out[0] = n_out[0];
        a.out[1] = n_out[1];
    }
}

} // namespace

hipError_t launch_seam(const SeamArgs &args, hipStream_t stream)
{
    const uint64_t P = args.boundary;
    if (P == 0 || P % kEpoch != 0 || args.g_begin < seam_first(P) || args.g_end > seam_end(P) || args.g_begin >= args.g_end || !args.out ||
        !args.synd)
        return hipErrorInvalidValue; // (bounds of every LDS array above)
    hipLaunchKernelGGL(seam_kernel, dim3(1), dim3(kSeamThreads), 0, stream, args);
    return hipGetLastError();
}

} // namespace adsb
