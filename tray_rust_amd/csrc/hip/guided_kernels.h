// The guided filter of tray_denoise_guided_device (include/trayhip.h states it): the dual-buffer NL-means of denoise_kernels.h whose weights are
// measured on one pair of films (the guide) and applied to another (the values). Both pairs are resolved by the unchanged k_dn_prepare<0> / <1>
// into records of their own, and k_gdn_filter reads the patch distances from the guide's records and the averaged colours from the values'.
// Device code only; compiled into libtrayhip_guided.so by guided.hip, and by g++ into the host emulation (tests/emu/emu_guided.cpp). All
// arithmetic is f32 and unfused (-ffp-contract=off).
//
// Scratch buffer (gdn_scratch_bytes = 96 bytes per pixel): n = width * height float4 records each,
//   [0, 3 n)    A4, B4, V4 of the values (even, odd)     (denoise_kernels.h: 48 bytes per pixel; V4 is written and not read)
//   [3 n, 6 n)  A4, B4, V4 of the guide (guide_a, guide_b)
// The two-pass call (gdn_two_pass_scratch_bytes = 128 bytes per pixel) puts the pilot between them:
//   [0, 3 n)    the values' records: tray_denoise_halves_device's scratch, which is what the guided filter needs of the values
//   [3 n, 5 n)  fa, fb: the first pass's cross-filtered halves as RGBW films
//   [5 n, 8 n)  the records of (fa, fb)
//
// k_gdn_filter is dn_filter_block with two sources. A workgroup of DN_BLOCK = 512 threads owns a 32 x 16 tile, stages the GUIDE'S records for the
// tile and its r + f halo in LDS (the arrays, their sizes and their banking are dn_filter_block's: 115 920 bytes at f = 3, one workgroup per CU)
// and walks the (2r+1)^2 offsets with the same three steps and the same two barriers per offset. What differs:
//   step 3  a(q), b(q) and valid(q) are the VALUES': two float4 loads per thread and offset from the values' records in global memory, issued at
//           the top of the offset's iteration, so that steps 1 and 2 and both barriers stand between the loads and their use. A half wave reads 32
//           consecutive records of one row (512 contiguous bytes per array); the tile's window of values is (32 + 2r) x (16 + 2r) x 32 bytes
//           (35 KB at r = 5) and stays in the CU's vector cache and in L2 after the first offsets. A q outside the image loads nothing and counts
//           as invalid, as a staged zero record does in dn_filter_block.
// Why not LDS: at r = 10, f = 3 the values' window beside the guide's region comes to 161 082 of gfx950's 163 840 bytes only with a validity
// bitmask and three float2 arrays of another layout than the guide's, i.e. a second staging loop and a second set of bank rules for 1.7 % of
// head room; one workgroup per CU fits either way, so LDS residency would buy no occupancy, only the latency that the early loads already hide.
// With the guide's records as the values' (the same films twice), every operation and its order are k_dn_filter's: the same bits.
// Barriers: the offset loop's bounds are uniform over the workgroup and the barriers sit outside every per-thread condition; a thread whose pixel
// lies outside the image runs to the end and stores nothing. Every global index is formed only after its bounds test.
#pragma once
#include "denoise_kernels.h"

namespace tr_guided {

using namespace tr_denoise;

__host__ __device__ inline uint64_t gdn_scratch_bytes(uint32_t width, uint32_t height) { return (uint64_t)width * height * 96u; }
__host__ __device__ inline uint64_t gdn_two_pass_scratch_bytes(uint32_t width, uint32_t height) { return (uint64_t)width * height * 128u; }

// guide, values: records of k_dn_prepare (3 n float4 each; of the values only A4 and B4 are read); out: n float4
template <int F>
__global__ __launch_bounds__(DN_BLOCK) void k_gdn_filter(const float4* __restrict__ guide, const float4* __restrict__ values, uint32_t width, uint32_t height,
                                                         uint32_t radius, float k, float4* __restrict__ out) {
    constexpr uint32_t EW = DN_TW + 2u * F, EH = DN_TH + 2u * F;   // the tile + f halo: where t is needed
    constexpr uint32_t N1 = (EW * EH + DN_BLOCK - 1u) / DN_BLOCK, N2 = (DN_TW * EH + DN_BLOCK - 1u) / DN_BLOCK;   // items per thread in steps 1 and 2
    __shared__ float4 s_a[DN_STAGE_MAX];   // the guide: (ga.r, ga.g, ga.b, gvalid)
    __shared__ float4 s_b[DN_STAGE_MAX];   // (gb.r, gb.g, gb.b, Vg.r)
    __shared__ float2 s_v[DN_STAGE_MAX];   // (Vg.g, Vg.b)
    __shared__ float2 s_t[EW * EH];        // (t_a, t_b) of the current offset ...
    __shared__ float s_p[EW * EH];         // ... and pair
    __shared__ float2 s_h[DN_TW * EH];     // their horizontal sums over 2f + 1 columns
    __shared__ float s_n[DN_TW * EH];
    const uint32_t tid = threadIdx.x;
    const int R = (int)radius, H = R + F;
    const uint32_t SW = DN_TW + 2u * (uint32_t)H, SH = DN_TH + 2u * (uint32_t)H;   // the staged region: SW * SH <= DN_STAGE_MAX as radius <= DN_RMAX
    const uint32_t tiles_x = dn_tiles_x(width);
    const int x0 = (int)((blockIdx.x % tiles_x) * DN_TW), y0 = (int)((blockIdx.x / tiles_x) * DN_TH);
    const size_t n = (size_t)width * height;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (uint32_t i = tid; i < SW * SH; i += DN_BLOCK) {
        const int gx = x0 - H + (int)(i % SW), gy = y0 - H + (int)(i / SW);
        float4 a = zero, b = zero, v = zero;
        if (gx >= 0 && gy >= 0 && gx < (int)width && gy < (int)height) {
            const size_t g = (size_t)gy * width + (size_t)gx;
            a = guide[g]; b = guide[n + g]; v = guide[2u * n + g];
        }
        s_a[i] = a; s_b[i] = make_float4(b.x, b.y, b.z, v.x); s_v[i] = make_float2(v.y, v.z);
    }
    __syncthreads();
    const uint32_t tx = tid % DN_TW, ty = tid / DN_TW;
    // this thread's items of steps 1 and 2 (the same for every offset): the staged index of p' and the first record of the row sum
    uint32_t ps[N1], hb[N2];
#pragma unroll
    for (uint32_t m = 0u; m < N1; ++m) {
        const uint32_t i = tid + m * DN_BLOCK;
        ps[m] = (i / EW + (uint32_t)R) * SW + i % EW + (uint32_t)R;
    }
#pragma unroll
    for (uint32_t m = 0u; m < N2; ++m) {
        const uint32_t i = tid + m * DN_BLOCK;
        hb[m] = (i / DN_TW) * EW + i % DN_TW;
    }
    const int px = x0 + (int)tx, py = y0 + (int)ty;   // this thread's output pixel, which may lie outside the image (partial tiles)
    const float k2 = k * k;
    float nar = 0.0f, nag = 0.0f, nab = 0.0f, da = 0.0f;   // A(p): weights from gb, applied to a
    float nbr = 0.0f, nbg = 0.0f, nbb = 0.0f, db = 0.0f;   // B(p): weights from ga, applied to b
    for (int dy = -R; dy <= R; ++dy)
        for (int dx = -R; dx <= R; ++dx) {
            const int shift = dy * (int)SW + dx;
            // the values at q, asked for now and used in step 3; outside the image: an invalid zero record
            const int qx = px + dx, qy = py + dy;
            float4 aq = zero, bq = zero;
            if (qx >= 0 && qy >= 0 && qx < (int)width && qy < (int)height) {
                const size_t g = (size_t)qy * width + (size_t)qx;
                aq = values[g]; bq = values[n + g];
            }
#pragma unroll
            for (uint32_t m = 0u; m < N1; ++m) {
                const uint32_t i = tid + m * DN_BLOCK;
                if (i < EW * EH) {
                    // (dn_filter_block's step 1 on the guide: no branch on pair, the product with it as the statement has it)
                    const uint32_t qs = (uint32_t)((int)ps[m] + shift);
                    const float4 ap = s_a[ps[m]], gq = s_a[qs], bp = s_b[ps[m]], hq = s_b[qs];
                    const float2 vp = s_v[ps[m]], vq = s_v[qs];
                    const float ta = (dn_term(ap.x, gq.x, bp.w, hq.w, k2) + dn_term(ap.y, gq.y, vp.x, vq.x, k2)) + dn_term(ap.z, gq.z, vp.y, vq.y, k2);
                    const float tb = (dn_term(bp.x, hq.x, bp.w, hq.w, k2) + dn_term(bp.y, hq.y, vp.x, vq.x, k2)) + dn_term(bp.z, hq.z, vp.y, vq.y, k2);
                    const float pair = ap.w * gq.w;
                    s_t[i] = make_float2(ta * pair, tb * pair);
                    s_p[i] = pair;
                }
            }
            __syncthreads();
#pragma unroll
            for (uint32_t m = 0u; m < N2; ++m) {
                const uint32_t i = tid + m * DN_BLOCK;
                if (i < DN_TW * EH) {
                    dn_f2 s = DN_LDS_F2(s_t, hb[m]);
                    float c = DN_LDS_F(s_p, hb[m]);
#pragma unroll
                    for (uint32_t j = 1u; j <= 2u * F; ++j) {
                        const dn_f2 t = DN_LDS_F2(s_t, hb[m] + j);
                        s.x = s.x + t.x; s.y = s.y + t.y; c = c + DN_LDS_F(s_p, hb[m] + j);
                    }
                    s_h[i] = make_float2(s.x, s.y);
                    s_n[i] = c;
                }
            }
            __syncthreads();   // (the next offset's step 1 writes s_t / s_p only; its barrier stands between this step 3 and the next step 2)
            dn_f2 s = DN_LDS_F2(s_h, tid);
            float c = DN_LDS_F(s_n, tid);
#pragma unroll
            for (uint32_t j = 1u; j <= 2u * F; ++j) {
                const dn_f2 t = DN_LDS_F2(s_h, tid + j * DN_TW);
                s.x = s.x + t.x; s.y = s.y + t.y; c = c + DN_LDS_F(s_n, tid + j * DN_TW);
            }
            if (c > 0.0f && aq.w != 0.0f) {
                const float div = 3.0f * c;
                const float d2a = s.x / div, d2b = s.y / div;
                const float wa = tr::ref_expf(-(d2a > 0.0f ? d2a : 0.0f)), wb = tr::ref_expf(-(d2b > 0.0f ? d2b : 0.0f));
                nar = nar + wb * aq.x; nag = nag + wb * aq.y; nab = nab + wb * aq.z; da = da + wb;
                nbr = nbr + wa * bq.x; nbg = nbg + wa * bq.y; nbb = nbb + wa * bq.z; db = db + wa;
            }
        }
    if (px >= (int)width || py >= (int)height) return;   // (after the last barrier)
    float4 A = zero, B = zero;
    if (da > 0.0f) A = make_float4(nar / da, nag / da, nab / da, 1.0f);
    if (db > 0.0f) B = make_float4(nbr / db, nbg / db, nbb / db, 1.0f);
    out[(size_t)py * width + (size_t)px] = make_float4((A.x + B.x) * 0.5f, (A.y + B.y) * 0.5f, (A.z + B.z) * 0.5f, 1.0f);
}

}  // namespace tr_guided
