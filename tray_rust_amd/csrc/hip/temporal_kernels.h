// The temporal filter of tray_denoise_temporal_device (include/trayhip.h states it): the dual-buffer NL-means of denoise_kernels.h with the windows
// of N neighbouring frames added to the centre frame's. Every frame is resolved by the unchanged k_dn_prepare<0> / <1> into records of its own,
// and k_tdn_pass adds one frame's window to the eight sums of every output pixel: once for the centre frame, then once per neighbour, in the
// caller's order. Device code only; compiled into libtrayhip_temporal.so by temporal.hip, and by g++ into the host emulation
// (tests/emu/emu_temporal.cpp). All arithmetic is f32 and unfused (-ffp-contract=off).
//
// Scratch buffer (tdn_scratch_bytes = 128 bytes per pixel, whatever N is): n = width * height float4 records each,
//   [0, 3 n)    A4, B4, V4 of the centre frame          (denoise_kernels.h: 48 bytes per pixel)
//   [3 n, 6 n)  A4, B4, V4 of the neighbour of the current pass
//   [6 n, 8 n)  the sums between passes: (sum w_b a, sum w_b) and (sum w_a b, sum w_a), not normalised
//
// k_tdn_pass is dn_filter_block with two sources. A workgroup of DN_BLOCK = 512 threads owns a 32 x 16 tile, stages the records of the PASS'S
// frame for the tile and its r + f halo in LDS (the arrays, their sizes and their banking are dn_filter_block's: 115 920 bytes at f = 3, one
// workgroup per CU) and walks the (2r+1)^2 offsets with the same three steps and the same two barriers per offset. What differs:
//   step 1  t(p', q') takes p' from the CENTRE frame and q' = p' + o from the pass's frame. A thread's p' are the same for every offset (N1 = 2
//           positions of the tile + f halo at f = 3), so their records are loaded from the centre's scratch once, before the loop, into
//           registers (10 floats each); only q' is read from LDS. A p' outside the image is an invalid zero record, as a staged one is.
//   step 3  a(q), b(q) and valid(q) are the pass's frame's.
//   sums    the eight sums start at 0 (first) or are read from `acc` (two float4 loads per thread); the last pass stores the normalised
//           ((A + B) / 2, 1) into `out`, every other pass stores the sums back. A thread reads and writes its own pixel's words only: no atomics,
//           every word written once per pass, the same bits in every run.
// With the centre as the pass's frame, first = last = 1, every operation and its order are k_dn_filter's: the same bits.
// Barriers: the offset loop's bounds are uniform over the workgroup and the barriers sit outside every per-thread condition; a thread whose pixel
// lies outside the image runs to the end, reads no sums and stores nothing.
#pragma once
#include "denoise_kernels.h"

namespace tr_temporal {

using namespace tr_denoise;

#define TDN_RMAX DN_RMAX   // the search radii of the centre's and the neighbours' windows: 1 ... 10, as k_dn_filter's (the staged region is the same)

__host__ __device__ inline uint64_t tdn_scratch_bytes(uint32_t width, uint32_t height) { return (uint64_t)width * height * 128u; }

// one pass: the window of `frame` (records of k_dn_prepare, 3 n float4) around every pixel, with the patches of `centre` (likewise; the same buffer
// in the centre's own pass) on the p side; acc: 2 n float4; out: n float4, written when last != 0
template <int F>
__global__ __launch_bounds__(DN_BLOCK) void k_tdn_pass(const float4* __restrict__ centre, const float4* __restrict__ frame, uint32_t width, uint32_t height,
                                                       uint32_t radius, float k, float4* __restrict__ acc, uint32_t first, uint32_t last,
                                                       float4* __restrict__ out) {
    constexpr uint32_t EW = DN_TW + 2u * F, EH = DN_TH + 2u * F;   // the tile + f halo: where t is needed
    constexpr uint32_t N1 = (EW * EH + DN_BLOCK - 1u) / DN_BLOCK, N2 = (DN_TW * EH + DN_BLOCK - 1u) / DN_BLOCK;   // items per thread in steps 1 and 2
    __shared__ float4 s_a[DN_STAGE_MAX];   // the pass's frame: (a.r, a.g, a.b, valid)
    __shared__ float4 s_b[DN_STAGE_MAX];   // (b.r, b.g, b.b, V.r)
    __shared__ float2 s_v[DN_STAGE_MAX];   // (V.g, V.b)
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
            a = frame[g]; b = frame[n + g]; v = frame[2u * n + g];
        }
        s_a[i] = a; s_b[i] = make_float4(b.x, b.y, b.z, v.x); s_v[i] = make_float2(v.y, v.z);
    }
    __syncthreads();
    const uint32_t tx = tid % DN_TW, ty = tid / DN_TW;
    // this thread's items of steps 1 and 2 (the same for every offset): the centre's records of p' in the staged layout, the staged index of p' (q' is
    // that plus the offset) and the first record of the row sum
    float4 pa[N1], pb[N1];
    float2 pv[N1];
    uint32_t ps[N1], hb[N2];
#pragma unroll
    for (uint32_t m = 0u; m < N1; ++m) {
        const uint32_t i = tid + m * DN_BLOCK;
        ps[m] = (i / EW + (uint32_t)R) * SW + i % EW + (uint32_t)R;
        const int gx = x0 - F + (int)(i % EW), gy = y0 - F + (int)(i / EW);
        float4 a = zero, b = zero, v = zero;
        if (i < EW * EH && gx >= 0 && gy >= 0 && gx < (int)width && gy < (int)height) {
            const size_t g = (size_t)gy * width + (size_t)gx;
            a = centre[g]; b = centre[n + g]; v = centre[2u * n + g];
        }
        pa[m] = a; pb[m] = make_float4(b.x, b.y, b.z, v.x); pv[m] = make_float2(v.y, v.z);
    }
#pragma unroll
    for (uint32_t m = 0u; m < N2; ++m) {
        const uint32_t i = tid + m * DN_BLOCK;
        hb[m] = (i / DN_TW) * EW + i % DN_TW;
    }
    const uint32_t pq = (ty + (uint32_t)H) * SW + tx + (uint32_t)H;   // the staged index of this thread's output pixel
    const uint32_t px = (uint32_t)x0 + tx, py = (uint32_t)y0 + ty;
    const bool inside = px < width && py < height;
    const size_t p = (size_t)py * width + px;
    const float k2 = k * k;
    float nar = 0.0f, nag = 0.0f, nab = 0.0f, da = 0.0f;   // A(p): weights from b, applied to a
    float nbr = 0.0f, nbg = 0.0f, nbb = 0.0f, db = 0.0f;   // B(p): weights from a, applied to b
    if (first == 0u && inside) {
        const float4 sa = acc[p], sb = acc[n + p];
        nar = sa.x; nag = sa.y; nab = sa.z; da = sa.w;
        nbr = sb.x; nbg = sb.y; nbb = sb.z; db = sb.w;
    }
    for (int dy = -R; dy <= R; ++dy)
        for (int dx = -R; dx <= R; ++dx) {
            const int shift = dy * (int)SW + dx;
#pragma unroll
            for (uint32_t m = 0u; m < N1; ++m) {
                const uint32_t i = tid + m * DN_BLOCK;
                if (i < EW * EH) {
                    // (dn_filter_block's step 1 with p' from registers: no branch on pair, the product with it as the statement has it)
                    const uint32_t qs = (uint32_t)((int)ps[m] + shift);
                    const float4 ap = pa[m], aq = s_a[qs], bp = pb[m], bq = s_b[qs];
                    const float2 vp = pv[m], vq = s_v[qs];
                    const float ta = (dn_term(ap.x, aq.x, bp.w, bq.w, k2) + dn_term(ap.y, aq.y, vp.x, vq.x, k2)) + dn_term(ap.z, aq.z, vp.y, vq.y, k2);
                    const float tb = (dn_term(bp.x, bq.x, bp.w, bq.w, k2) + dn_term(bp.y, bq.y, vp.x, vq.x, k2)) + dn_term(bp.z, bq.z, vp.y, vq.y, k2);
                    const float pair = ap.w * aq.w;
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
            const uint32_t qs = (uint32_t)((int)pq + shift);
            const float4 aq = s_a[qs];
            if (c > 0.0f && aq.w != 0.0f) {
                const float4 bq = s_b[qs];
                const float div = 3.0f * c;
                const float d2a = s.x / div, d2b = s.y / div;
                const float wa = tr::ref_expf(-(d2a > 0.0f ? d2a : 0.0f)), wb = tr::ref_expf(-(d2b > 0.0f ? d2b : 0.0f));
                nar = nar + wb * aq.x; nag = nag + wb * aq.y; nab = nab + wb * aq.z; da = da + wb;
                nbr = nbr + wa * bq.x; nbg = nbg + wa * bq.y; nbb = nbb + wa * bq.z; db = db + wa;
            }
        }
    if (!inside) return;   // (after the last barrier)
    if (last != 0u) {
        float4 A = zero, B = zero;
        if (da > 0.0f) A = make_float4(nar / da, nag / da, nab / da, 1.0f);
        if (db > 0.0f) B = make_float4(nbr / db, nbg / db, nbb / db, 1.0f);
        out[p] = make_float4((A.x + B.x) * 0.5f, (A.y + B.y) * 0.5f, (A.z + B.z) * 0.5f, 1.0f);
    } else {
        acc[p] = make_float4(nar, nag, nab, da);
        acc[n + p] = make_float4(nbr, nbg, nbb, db);
    }
}

}  // namespace tr_temporal
