// The kernels that let tray_render_noise_target_filtered_device stop on the error of the denoised image (include/trayhip.h): k_dn_filter_halves
// writes the two cross-filtered halves of the dual-buffer filter as films of their own, over the whole frame or over a list of 32 x 16 blocks;
// k_guide_mark and k_guide_compact make the next round's list from the active tiles. Device code only; compiled into libtrayhip_guide.so by
// guide.hip, and by g++ into the host emulation (tests/emu/emu_guide.cpp).
//
// k_dn_filter_halves is k_dn_filter (denoise_kernels.h, which documents the algorithm, the LDS layout and the banking) with another end: the
// staging, the two barriers per offset, the separable patch sums and every sum in its order are that kernel's, line for line, and where it
// stores ((A + B) / 2, 1) this one stores fa = (A, wA) and fb = (B, wB), two float4 stores per thread. (fa.rgb + fb.rgb) * 0.5f is therefore
// k_dn_filter's out.rgb to the bit. The body is carried here and not shared through a function template of denoise_kernels.h: lifting it there
// moves libtrayhip_denoise.so's code objects (another schedule of the same instructions), and that library's recorded hash stands for its GPU run.
// A change of k_dn_filter's arithmetic must be made in both; tests/test_guide_emu.py and tests/test_gpu_guide.py compare the two bit for bit.
// Barriers: a workgroup takes its block index from the list (or blockIdx.x); an index outside the frame's blocks ends the whole workgroup before
// the first barrier, and in every other workgroup the loops over offsets and items have uniform bounds, so every thread of a workgroup reaches
// every barrier whatever the list holds. Stores are bounded by the image.
#pragma once
#include "denoise_kernels.h"

namespace tr_guide {

using namespace tr_denoise;

#define GD_MARK_BLOCK 256u      // k_guide_mark: one thread per queue entry
#define GD_COMPACT_BLOCK 1024u  // k_guide_compact: the one workgroup

template <int F>
__global__ __launch_bounds__(DN_BLOCK) void k_dn_filter_halves(const float4* __restrict__ scratch, uint32_t width, uint32_t height, uint32_t radius,
                                                               float k, const uint32_t* __restrict__ blocks, float4* __restrict__ fa,
                                                               float4* __restrict__ fb) {
    const uint32_t block = blocks ? blocks[blockIdx.x] : blockIdx.x;
    if (block >= dn_tiles_x(width) * dn_tiles_y(height)) return;   // (the same for every thread of the workgroup)
    constexpr uint32_t EW = DN_TW + 2u * F, EH = DN_TH + 2u * F;   // the tile + f halo: where t is needed
    constexpr uint32_t N1 = (EW * EH + DN_BLOCK - 1u) / DN_BLOCK, N2 = (DN_TW * EH + DN_BLOCK - 1u) / DN_BLOCK;   // items per thread in steps 1 and 2
    __shared__ float4 s_a[DN_STAGE_MAX];   // (a.r, a.g, a.b, valid)
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
    const int x0 = (int)((block % tiles_x) * DN_TW), y0 = (int)((block / tiles_x) * DN_TH);
    const size_t n = (size_t)width * height;
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (uint32_t i = tid; i < SW * SH; i += DN_BLOCK) {
        const int gx = x0 - H + (int)(i % SW), gy = y0 - H + (int)(i / SW);
        float4 a = zero, b = zero, v = zero;
        if (gx >= 0 && gy >= 0 && gx < (int)width && gy < (int)height) {
            const size_t g = (size_t)gy * width + (size_t)gx;
            a = scratch[g]; b = scratch[n + g]; v = scratch[2u * n + g];
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
    const uint32_t pq = (ty + (uint32_t)H) * SW + tx + (uint32_t)H;   // the staged index of this thread's output pixel
    const float k2 = k * k;
    float nar = 0.0f, nag = 0.0f, nab = 0.0f, da = 0.0f;   // A(p): weights from b, applied to a
    float nbr = 0.0f, nbg = 0.0f, nbb = 0.0f, db = 0.0f;   // B(p): weights from a, applied to b
    for (int dy = -R; dy <= R; ++dy)
        for (int dx = -R; dx <= R; ++dx) {
            const int shift = dy * (int)SW + dx;
#pragma unroll
            for (uint32_t m = 0u; m < N1; ++m) {
                const uint32_t i = tid + m * DN_BLOCK;
                if (i < EW * EH) {
                    // (no branch on pair, and the product with it as the statement has it: an invalid or outside position holds a = b = 0 and a
                    // finite V, so t is finite and t * 0 drops it; every component of the records is used, so each is one ds_read_b128 / _b64)
                    const uint32_t qs = (uint32_t)((int)ps[m] + shift);
                    const float4 ap = s_a[ps[m]], aq = s_a[qs], bp = s_b[ps[m]], bq = s_b[qs];
                    const float2 vp = s_v[ps[m]], vq = s_v[qs];
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
    const uint32_t px = (uint32_t)x0 + tx, py = (uint32_t)y0 + ty;
    if (px < width && py < height) {
        float4 A = zero, B = zero;
        if (da > 0.0f) A = make_float4(nar / da, nag / da, nab / da, 1.0f);
        if (db > 0.0f) B = make_float4(nbr / db, nbg / db, nbb / db, 1.0f);
        fa[(size_t)py * width + px] = A;
        fb[(size_t)py * width + px] = B;
    }
}

// The 32 x 16 blocks that hold a tile of queue[0, n) whose flag is set (active == null: every tile of the queue): flags[block] = 1, the block
// row-major over blocks_x blocks per row. A block holds 4 x 2 tiles of 8 x 8 pixels. Several threads may store the same word; all store 1.
// Tiles whose block lies outside the blocks_x x blocks_y grid are passed over.
__global__ __launch_bounds__(GD_MARK_BLOCK) void k_guide_mark(const uint2* __restrict__ queue, const uint32_t* __restrict__ active, uint32_t n,
                                                              uint32_t blocks_x, uint32_t blocks_y, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * GD_MARK_BLOCK + threadIdx.x;
    if (i >= n || (active && active[i] == 0u)) return;
    const uint2 tile = queue[i];
    const uint32_t bx = tile.x / (DN_TW / 8u), by = tile.y / (DN_TH / 8u);
    if (bx < blocks_x && by < blocks_y) flags[by * blocks_x + bx] = 1u;
}

// The indices of the set flags of flags[0, n) in rising order into list, their number into *count: k_noise_compact's scan (noise_kernels.h) --
// one workgroup walks the flags in steps of GD_COMPACT_BLOCK, a ballot per wave, the waves' counts through LDS.
__global__ __launch_bounds__(GD_COMPACT_BLOCK) void k_guide_compact(const uint32_t* __restrict__ flags, uint32_t n, uint32_t* __restrict__ list,
                                                                    uint32_t* __restrict__ count) {
    __shared__ uint32_t s_wave[GD_COMPACT_BLOCK / 64u];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t total = 0u;   // entries written before this step (the same in every thread)
    for (uint32_t i0 = 0u; i0 < n; i0 += GD_COMPACT_BLOCK) {
        const uint32_t i = i0 + threadIdx.x;
        const bool keep = i < n && flags[i] != 0u;
        const unsigned long long m = __ballot(keep);
        if (lane == 0u) s_wave[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0u, sum = 0u;
        for (uint32_t k = 0u; k < GD_COMPACT_BLOCK / 64u; ++k) {
            const uint32_t c = s_wave[k];
            before += k < wave ? c : 0u;
            sum += c;
        }
        if (keep) list[total + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = i;   // (an index < n: at most one entry per flag)
        total += sum;
        __syncthreads();   // (s_wave is rewritten by the next step)
    }
    if (threadIdx.x == 0u) *count = total;
}

}  // namespace tr_guide
