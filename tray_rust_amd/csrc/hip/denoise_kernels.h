// The dual-buffer non-local-means filter of tray_denoise_device (include/trayhip.h states the filter): k_dn_prepare resolves the two films into
// float4 records of the scratch buffer, dn_filter_block computes the sums of the two cross-filtered halves of one tile from them, and k_dn_filter
// stores the halves' mean as the output image. dn_filter_block is the one body of the filter: k_dn_filter_halves (guide_kernels.h), k_tdn_pass
// (temporal_kernels.h) and k_gdn_filter (guided_kernels.h) are other fronts and ends around it. Device code only; compiled into
// libtrayhip_denoise.so, _guide.so, _temporal.so and _guided.so by denoise.hip, guide.hip, temporal.hip and guided.hip, and by g++ into the host
// emulation (tests/emu/emu_denoise.cpp, emu_guide.cpp, emu_temporal.cpp, emu_guided.cpp). All arithmetic is f32 and unfused (-ffp-contract=off).
//
// Scratch buffer (tray_denoise_scratch_bytes = 48 bytes per pixel): three arrays of width * height float4 records,
//   A4[p] = (a.r, a.g, a.b, valid ? 1 : 0)      a = E.rgb / E.w where valid, else 0
//   B4[p] = (b.r, b.g, b.b, 0)                  b = O.rgb / O.w where valid, else 0
//   V4[p] = (V.r, V.g, V.b, 0)                  the 3 x 3 mean of (a - b)^2 / 2 over the valid pixels
//
// dn_filter_block. A workgroup of DN_BLOCK = 512 threads (8 waves) owns a DN_TW x DN_TH = 32 x 16 tile of the output, one pixel per thread. It
// stages the records of the tile and its halo of H = r + f pixels in LDS once (positions outside the image as invalid zeros: one HBM read per
// staged pixel), then walks the (2r+1)^2 offsets o. For each offset, between two barriers each:
//   1. t of both buffers and `pair`, once per pixel of the tile + f halo ((32 + 2f) x (16 + 2f) positions: 836 at f = 3, 1.63 per output pixel),
//      into s_t = (t_a, t_b) and s_p = pair: both buffers in one pass, since they share V, pair and |N|;
//   2. the horizontal sums of 2f + 1 entries for the 32 columns of every row of the tile + f halo, into s_h / s_n;
//   3. per output pixel the vertical sum of 2f + 1 entries of s_h / s_n, the two weights and the four accumulations, in registers.
// The patch sum is 2 (2f + 1) adds per quantity instead of (2f + 1)^2. A thread's items of steps 1 and 2 are the same for every offset, so their
// LDS indices are computed once. Sums run in a fixed order and every output pixel is written once by one thread: the same bits in every run.
// LDS per workgroup (static, sized for r = 10, f = 3): the staged region of 58 x 42 pixels as s_a = (a, valid) and s_b = (b, V.r), 16 bytes each,
// and s_v = (V.g, V.b), 8 bytes: 97 440 bytes; s_t + s_p 10 032 and s_h + s_n 8 448 bytes at f = 3: 115 920 of gfx950's 163 840 bytes, so one
// workgroup (8 waves, 2 per SIMD) per CU at every radius; the registers (69 VGPRs at f = 3; 76 with DN_P_CENTRE, 77 with DN_Q_GLOBAL) would
// allow six or seven.
// Banking: every component of every record is used where it is read, so the staged records are read with ds_read_b128 / ds_read_b64 and the
// sums with ds_read_b64 / ds_read_b32 (DN_LDS_F2 / DN_LDS_F below keep them single reads). In steps 2 and 3 and in step 3's reads of the
// staged arrays each 32-lane half of a wave reads 32 consecutive entries of one row (contiguous bytes: conflict-free); step 1 walks rows of
// 32 + 2f positions, so a wave's reads wrap to the next staged row once or twice, where two lanes of a group can meet on a bank (2-way at
// worst, on those instructions only).
// Two sources. Two compile-time switches (dn_p_side, dn_q_values below) let the records of the two sides of a weight come from elsewhere than the
// staged frame; everything else -- the arrays, the staging loop, the three steps, both barriers, the order of every sum -- is the same code:
//   DN_P_CENTRE  p' of step 1 comes from the records of another frame, `centre` (the temporal filter: patches of the centre frame against the
//                staged neighbour). A thread's p' are the same for every offset (N1 = 2 positions at f = 3), so their records are loaded once,
//                before the offset loop, into registers (10 floats each); only q' is read from LDS.
//   DN_Q_GLOBAL  a(q), b(q) and valid(q) of step 3 come from the records of other films, `values` (the guided filter: weights measured on the
//                staged guide, applied to the values): two float4 loads per thread and offset, issued at the top of the offset's iteration, so
//                that steps 1 and 2 and both barriers stand between the loads and their use. A q outside the image loads nothing and counts
//                as invalid, as a staged zero record does; every global index is formed only after its bounds test.
// The eight sums start at 0 or, given `acc`, at the sums an earlier pass stored (read after the staging barrier, by threads inside the image
// only): the accumulators' initial values, so that the additions run in the order of one longer window.
// Barriers: dn_filter_block owns the LDS arrays and both barriers per offset, so EVERY thread of the workgroup must call it, under control flow
// that is uniform over the workgroup. Inside it the loops over offsets and items have uniform bounds, no barrier sits inside a per-thread
// condition, and a thread whose pixel lies outside the image runs to the end like any other (it reads no `acc`, and its caller skips the
// store). k_dn_filter, k_tdn_pass and k_gdn_filter call it unconditionally; k_dn_filter_halves either returns with the whole workgroup before
// the call (a listed block outside the frame: the test reads no per-thread value) or calls it.
#pragma once
#include <stdint.h>
#include <type_traits>
#ifndef TR_DEV
#define TR_DEV __device__ __forceinline__
#endif
#include "dev_libm.h"   // tr::ref_expf: glibc's expf restated, the same bits on the device and in the emulation

namespace tr_denoise {

#define DN_PREP_BLOCK 256u   // k_dn_prepare: one thread per pixel
#define DN_BLOCK 512u        // k_dn_filter: one thread per pixel of the tile
#define DN_TW 32u
#define DN_TH 16u
#define DN_RMAX 10u          // search radius r: 1 ... DN_RMAX (run-time)
#define DN_FMAX 3u           // patch radius f: 0 ... DN_FMAX (template argument)
#define DN_HMAX (DN_RMAX + DN_FMAX)
#define DN_STAGE_MAX ((DN_TW + 2u * DN_HMAX) * (DN_TH + 2u * DN_HMAX))   // 58 x 42 staged records
#define DN_EPS 1e-7f

// workgroups of k_dn_filter for a width x height image (one per tile, row by row), and the bytes of scratch (three float4 records per pixel)
__host__ __device__ inline uint32_t dn_tiles_x(uint32_t width) { return (width + DN_TW - 1u) / DN_TW; }
__host__ __device__ inline uint32_t dn_tiles_y(uint32_t height) { return (height + DN_TH - 1u) / DN_TH; }
__host__ __device__ inline uint64_t dn_scratch_bytes(uint32_t width, uint32_t height) { return (uint64_t)width * height * 48u; }

// The reads of the patch sums: 2f + 1 records at constant distances per thread, which the backend would pair into ds_read2_b64 / ds_read2_b32 --
// forms that cost four / two times the LDS cycles of the single ds_read_b64 / ds_read_b32 per byte (MI355X: 16 cycles per ds_read2_b64 against 2
// per ds_read_b64). Volatile reads through the LDS address space stay single reads. The host emulation reads the arrays as they are.
#ifdef TR_HOST_EMU
typedef float2 dn_f2;
#define DN_LDS_F2(arr, i) ((arr)[i])
#define DN_LDS_F(arr, i) ((arr)[i])
#else
typedef float dn_f2 __attribute__((ext_vector_type(2)));
#define DN_LDS_F2(arr, i) (*(const volatile __attribute__((address_space(3))) tr_denoise::dn_f2*)&(arr)[i])
#define DN_LDS_F(arr, i) (*(const volatile __attribute__((address_space(3))) float*)&(arr)[i])
#endif

TR_DEV bool dn_finite(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
TR_DEV bool dn_finite4(float4 v) { return dn_finite(v.x) && dn_finite(v.y) && dn_finite(v.z) && dn_finite(v.w); }

// PASS 0: A4 and B4 of pixel p from one float4 load per film. PASS 1 (a second launch, after pass 0 is complete): V4 of pixel p from the A4 / B4
// records of its 3 x 3 box, summed row by row; (a - b)^2 / 2 is 0 at an invalid pixel, whose a and b are 0.
template <int PASS>
__global__ __launch_bounds__(DN_PREP_BLOCK) void k_dn_prepare(const float4* __restrict__ even, const float4* __restrict__ odd, uint32_t width,
                                                              uint32_t height, float4* __restrict__ scratch) {
    const size_t n = (size_t)width * height;
    const size_t p = (size_t)blockIdx.x * DN_PREP_BLOCK + threadIdx.x;
    if (p >= n) return;
    float4* const A4 = scratch;
    float4* const B4 = scratch + n;
    if (PASS == 0) {
        const float4 E = even[p], O = odd[p];
        const bool valid = E.w > 0.0f && O.w > 0.0f && dn_finite4(E) && dn_finite4(O);
        float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
        if (valid) {
            a = make_float4(E.x / E.w, E.y / E.w, E.z / E.w, 1.0f);
            b = make_float4(O.x / O.w, O.y / O.w, O.z / O.w, 0.0f);
        }
        A4[p] = a;
        B4[p] = b;
    } else {
        float4* const V4 = scratch + 2u * n;
        const int x = (int)(p % width), y = (int)(p / width);
        float sr = 0.0f, sg = 0.0f, sb = 0.0f, cnt = 0.0f;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                const int qx = x + dx, qy = y + dy;
                if (qx < 0 || qy < 0 || qx >= (int)width || qy >= (int)height) continue;
                const size_t q = (size_t)qy * width + (size_t)qx;
                const float4 a = A4[q], b = B4[q];
                const float dr = a.x - b.x, dg = a.y - b.y, db = a.z - b.z;
                sr = sr + dr * dr * 0.5f;
                sg = sg + dg * dg * 0.5f;
                sb = sb + db * db * 0.5f;
                cnt = cnt + a.w;
            }
        V4[p] = cnt > 0.0f ? make_float4(sr / cnt, sg / cnt, sb / cnt, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
}

// one channel's term of t(p', q'): ((x(p') - x(q'))^2 - (V(p') + min(V(p'), V(q')))) / (eps + k^2 (V(p') + V(q')))
TR_DEV float dn_term(float xp, float xq, float vp, float vq, float k2) {
    const float d = xp - xq;
    return (d * d - (vp + (vp < vq ? vp : vq))) / (DN_EPS + k2 * (vp + vq));
}

// the two filtered halves of one output pixel: A = even filtered with odd's weights, B the other way round, each (rgb, 1), or zeros where no
// weight was collected; (px, py): the pixel, which may lie outside the image (partial tiles) -- the caller stores only inside it
struct dn_halves { float4 A, B; uint32_t px, py; };

// what dn_filter_block returns: the eight sums of one output pixel, not normalised, as the two records the temporal filter keeps between its
// passes -- A = (sum w_b a, sum w_b), B = (sum w_a b, sum w_a) --, and the pixel as dn_halves has it
struct dn_sums { float4 A, B; uint32_t px, py; };

TR_DEV dn_halves dn_normalise(const dn_sums& s) {
    const float4 zero = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    dn_halves h = {zero, zero, s.px, s.py};
    if (s.A.w > 0.0f) h.A = make_float4(s.A.x / s.A.w, s.A.y / s.A.w, s.A.z / s.A.w, 1.0f);
    if (s.B.w > 0.0f) h.B = make_float4(s.B.x / s.B.w, s.B.y / s.B.w, s.B.z / s.B.w, 1.0f);
    return h;
}

// the output pixel of the filter: ((A + B) / 2, 1)
TR_DEV float4 dn_mean(const dn_halves& h) { return make_float4((h.A.x + h.B.x) * 0.5f, (h.A.y + h.B.y) * 0.5f, (h.A.z + h.B.z) * 0.5f, 1.0f); }

// The two compile-time switches of dn_filter_block (the file comment, "Two sources").
enum dn_p_side { DN_P_STAGED, DN_P_CENTRE };     // p' of step 1: the staged records / the records of `centre`, held in registers
enum dn_q_values { DN_Q_STAGED, DN_Q_GLOBAL };   // a(q), b(q), valid(q) of step 3: the staged records / the records of `values` in global memory

// The sums of the calling thread's pixel of tile `block` (row-major over dn_tiles_x(width) tiles per row; block < dn_tiles_x * dn_tiles_y) over
// the window of `staged` (records of k_dn_prepare, 3 n float4). centre: the records of the p' side (DN_P_CENTRE; else unused); values: those
// of a(q), b(q) (DN_Q_GLOBAL; else unused; their V4 is not read); acc: null, or 2 n float4 of sums to start from. Called by all DN_BLOCK
// threads of a workgroup together (above).
template <int F, dn_p_side PS = DN_P_STAGED, dn_q_values QV = DN_Q_STAGED>
TR_DEV dn_sums dn_filter_block(const float4* __restrict__ staged, const float4* __restrict__ centre, const float4* __restrict__ values, uint32_t width,
                               uint32_t height, uint32_t radius, float k, uint32_t block, const float4* acc) {
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
            a = staged[g]; b = staged[n + g]; v = staged[2u * n + g];
        }
        s_a[i] = a; s_b[i] = make_float4(b.x, b.y, b.z, v.x); s_v[i] = make_float2(v.y, v.z);
    }
    __syncthreads();
    const uint32_t tx = tid % DN_TW, ty = tid / DN_TW;
    // this thread's items of steps 1 and 2 (the same for every offset): the staged index of p' (q' is that plus the offset), with DN_P_CENTRE the
    // centre's records of p' in the staged layout (an item past the tile + f halo or a position outside the image: an invalid zero record), and
    // the first record of the row sum
    uint32_t ps[N1], hb[N2];
    float4 pa[N1], pb[N1];
    float2 pv[N1];
#pragma unroll
    for (uint32_t m = 0u; m < N1; ++m) {
        const uint32_t i = tid + m * DN_BLOCK;
        ps[m] = (i / EW + (uint32_t)R) * SW + i % EW + (uint32_t)R;
        if constexpr (PS == DN_P_CENTRE) {
            const int gx = x0 - F + (int)(i % EW), gy = y0 - F + (int)(i / EW);
            float4 a = zero, b = zero, v = zero;
            if (i < EW * EH && gx >= 0 && gy >= 0 && gx < (int)width && gy < (int)height) {
                const size_t g = (size_t)gy * width + (size_t)gx;
                a = centre[g]; b = centre[n + g]; v = centre[2u * n + g];
            }
            pa[m] = a; pb[m] = make_float4(b.x, b.y, b.z, v.x); pv[m] = make_float2(v.y, v.z);
        }
    }
#pragma unroll
    for (uint32_t m = 0u; m < N2; ++m) {
        const uint32_t i = tid + m * DN_BLOCK;
        hb[m] = (i / DN_TW) * EW + i % DN_TW;
    }
    const uint32_t pq = (ty + (uint32_t)H) * SW + tx + (uint32_t)H;   // the staged index of this thread's output pixel
    const uint32_t px = (uint32_t)x0 + tx, py = (uint32_t)y0 + ty;    // the pixel, which may lie outside the image (partial tiles)
    const float k2 = k * k;
    float nar = 0.0f, nag = 0.0f, nab = 0.0f, da = 0.0f;   // A(p): weights from b, applied to a
    float nbr = 0.0f, nbg = 0.0f, nbb = 0.0f, db = 0.0f;   // B(p): weights from a, applied to b
    if (acc && px < width && py < height) {
        const size_t p = (size_t)py * width + px;
        const float4 sa = acc[p], sb = acc[n + p];
        nar = sa.x; nag = sa.y; nab = sa.z; da = sa.w;
        nbr = sb.x; nbg = sb.y; nbb = sb.z; db = sb.w;
    }
    for (int dy = -R; dy <= R; ++dy)
        for (int dx = -R; dx <= R; ++dx) {
            const int shift = dy * (int)SW + dx;
            float4 aq = zero, bq = zero;   // a(q), b(q) of step 3
            if constexpr (QV == DN_Q_GLOBAL) {
                // asked for now and used in step 3; outside the image: an invalid zero record
                const int qx = (int)px + dx, qy = (int)py + dy;
                if (qx >= 0 && qy >= 0 && qx < (int)width && qy < (int)height) {
                    const size_t g = (size_t)qy * width + (size_t)qx;
                    aq = values[g]; bq = values[n + g];
                }
            }
#pragma unroll
            for (uint32_t m = 0u; m < N1; ++m) {
                const uint32_t i = tid + m * DN_BLOCK;
                if (i < EW * EH) {
                    // (no branch on pair, and the product with it as the statement has it: an invalid or outside position holds a = b = 0 and a
                    // finite V, so t is finite and t * 0 drops it; every component of the records is used, so each is one ds_read_b128 / _b64)
                    const uint32_t qs = (uint32_t)((int)ps[m] + shift);
                    float4 ap, bp;
                    float2 vp;
                    if constexpr (PS == DN_P_CENTRE) { ap = pa[m]; bp = pb[m]; vp = pv[m]; }
                    else { ap = s_a[ps[m]]; bp = s_b[ps[m]]; vp = s_v[ps[m]]; }
                    const float4 gq = s_a[qs], hq = s_b[qs];
                    const float2 vq = s_v[qs];
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
            const uint32_t qs = (uint32_t)((int)pq + shift);
            if constexpr (QV == DN_Q_STAGED) aq = s_a[qs];
            if (c > 0.0f && aq.w != 0.0f) {
                if constexpr (QV == DN_Q_STAGED) bq = s_b[qs];
                const float div = 3.0f * c;
                const float d2a = s.x / div, d2b = s.y / div;
                const float wa = tr::ref_expf(-(d2a > 0.0f ? d2a : 0.0f)), wb = tr::ref_expf(-(d2b > 0.0f ? d2b : 0.0f));
                nar = nar + wb * aq.x; nag = nag + wb * aq.y; nab = nab + wb * aq.z; da = da + wb;
                nbr = nbr + wa * bq.x; nbg = nbg + wa * bq.y; nbb = nbb + wa * bq.z; db = db + wa;
            }
        }
    return dn_sums{make_float4(nar, nag, nab, da), make_float4(nbr, nbg, nbb, db), px, py};
}

// one workgroup per tile of the image, row by row: out = ((A + B) / 2, 1)
template <int F>
__global__ __launch_bounds__(DN_BLOCK) void k_dn_filter(const float4* __restrict__ scratch, uint32_t width, uint32_t height, uint32_t radius, float k,
                                                        float4* __restrict__ out) {
    const dn_sums s = dn_filter_block<F>(scratch, nullptr, nullptr, width, height, radius, k, blockIdx.x, nullptr);
    if (s.px < width && s.py < height) out[(size_t)s.py * width + s.px] = dn_mean(dn_normalise(s));
}

// Host side: fn(std::integral_constant<int, F>()) for the F that patch selects (0 ... DN_FMAX; the callers have checked the range), and what it
// returns: the one place where the run-time patch radius becomes the template argument of k_dn_filter / k_dn_filter_halves.
template <class Fn>
inline auto dn_with_patch(uint32_t patch, Fn&& fn) {
    switch (patch) {
        case 0u: return fn(std::integral_constant<int, 0>());
        case 1u: return fn(std::integral_constant<int, 1>());
        case 2u: return fn(std::integral_constant<int, 2>());
        default: return fn(std::integral_constant<int, 3>());
    }
}

}  // namespace tr_denoise
