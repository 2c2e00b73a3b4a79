// Kernels of libtrayhip_firsthit.so (include/trayhip.h: tray_render_first_hit_device, tray_debug_first_hit, tray_denoise_demodulated_device).
// Included behind kernels.hip (first_hit.hip; tests/emu/emu_first_hit.cpp), whose camera, traversal, hit and film functions they call: the
// first hit of a camera sample is the position, the ray and the closest hit the tile kernel traces for that sample, written through the same
// RenderTarget::write into three films of its own.
#pragma once

#define FH_PLANES 10   // albedo rgb, normal xyz, depth (t, hit, 0), weight: the planes of the tile's LDS window
#define FH_WIN_FLOATS (FH_PLANES * WIN_PLANE)

// what one camera sample contributes: the nine colour words of its three films
struct FirstHit { float c[9]; };

// the first-hit albedo of a hit's material: c0 of MATTE and PLASTIC -- the constant, or tex_c0 at the hit's (u, v, ray.time) as
// resolve_textured samples it --, 1 for every other kind and for an instance without a material
TR_DEV f3 fh_albedo(const DevScene& sc, const Hit& h, float time) {
    const uint32_t mid = sc.instances[h.inst].material_id;
    if (mid == 0xffffffffu) return mk(1.0f, 1.0f, 1.0f);
    const DevMaterial* __restrict__ m = sc.materials + mid;
    if (m->mat_kind != TRAY_MAT_MATTE && m->mat_kind != TRAY_MAT_PLASTIC) return mk(1.0f, 1.0f, 1.0f);
    if (m->tex_c0 != TRAY_NO_TEXTURE) { const Rgba c = texture_sample(sc, m->tex_c0, h.u, h.v, time); return mk(c.r, c.g, c.b); }
    return mk(m->c0[0], m->c0[1], m->c0[2]);
}

// camera ray of one sample, traced by the whole wave (cooperative leaf test inside the traversal); `active`: this lane's sample counts
template <int ANIM>
TR_DEV FirstHit fh_sample(const DevScene& sc, const DevScene* __restrict__ scp, uint32_t* __restrict__ my_stack, float sx, float sy, float t, bool active) {
    const Ray r = camera_ray<ANIM>(sc, sx, sy, t);
    const TraceResult tr_ = trace<ANIM>(scp, my_stack, r, false, active);
    FirstHit o;
#pragma unroll
    for (int k = 0; k < 9; ++k) o.c[k] = 0.0f;
    if (active && tr_.hit) {
        const Hit h = finish_hit<ANIM>(sc, r, tr_.rec);
        const f3 a = fh_albedo(sc, h, r.time);
        o.c[0] = a.x; o.c[1] = a.y; o.c[2] = a.z;
        o.c[3] = h.n.x; o.c[4] = h.n.y; o.c[5] = h.n.z;
        o.c[6] = tr_.rec.t; o.c[7] = 1.0f;
    }
    return o;
}

// RenderTarget::write of one sample into the ten planes of the window (film_splat with nine colours): footprint and filter weight once
TR_DEV void fh_splat(const DevScene& sc, float* __restrict__ s_win, const float* __restrict__ s_table, int x0, int y0, float sx, float sy,
                     const FirstHit& v) {
    const int fpw = sc.fpw, fph = sc.fph;
    const int xr0 = max(x0 - fpw, 0), xr1 = min(x0 + 8 + fpw, (int)sc.width - 1);
    const int yr0 = max(y0 - fph, 0), yr1 = min(y0 + 8 + fph, (int)sc.height - 1);
    const float img_x = sx - 0.5f, img_y = sy - 0.5f;
    int ix_lo, ix_hi, iy_lo, iy_hi;
    film_admit(sx, xr0, xr1, fpw, ix_lo, ix_hi);
    film_admit(sy, yr0, yr1, fph, iy_lo, iy_hi);
    const int wx0 = x0 - fpw, wy0 = y0 - fph;
    for (int iy = iy_lo; iy <= iy_hi; ++iy) {
        const float fy = fabsf((float)iy - img_y) * sc.inv_h;
        if (fy > sc.filter_h) continue;
        const int fy_idx = min((int)(fy * (float)TRAY_FILTER_TABLE_SIZE), TRAY_FILTER_TABLE_SIZE - 1);
        for (int ix = ix_lo; ix <= ix_hi; ++ix) {
            const float fx = fabsf((float)ix - img_x) * sc.inv_w;
            if (fx > sc.filter_w) continue;
            const int fx_idx = min((int)(fx * (float)TRAY_FILTER_TABLE_SIZE), TRAY_FILTER_TABLE_SIZE - 1);
            const float weight = s_table[fy_idx * TRAY_FILTER_TABLE_SIZE + fx_idx];
            const int o = (iy - wy0) * WIN_STRIDE + (ix - wx0);
#pragma unroll
            for (int k = 0; k < 9; ++k) atomicAdd(&s_win[o + k * WIN_PLANE], weight * v.c[k]);
            atomicAdd(&s_win[o + 9 * WIN_PLANE], weight);
        }
    }
}

// One workgroup per 8 x 8 tile of the list: lane l of every wave owns pixel l of the tile, wave w takes the samples smp_begin + w, + 4, ... below
// smp_end, so every trace is made by whole waves under wave-uniform control flow; a wave with fewer samples leaves its loop earlier. The
// tile's ten planes live in LDS and are added to the three films once, after a barrier every thread reaches.
template <int ANIM>
__global__ __launch_bounds__(TR_BLOCK) void k_first_hit_tiles(const DevScene scv, const uint2* __restrict__ tiles, uint32_t spp, uint32_t kf,
                                                              uint32_t smp_begin, uint32_t smp_end, float* __restrict__ albedo,
                                                              float* __restrict__ normal, float* __restrict__ depth) {
    TR_DYN_LDS(uint32_t, s_stack);   // stack_depth x TR_BLOCK entries (and the cooperative leaf test's area), sized per scene at launch
    __shared__ float s_win[FH_WIN_FLOATS];
    const DevScene& sc = scv;
    const DevScene* const scp = &scv;
    const float* __restrict__ const s_table = sc_filter_table(scv);
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint32_t i = tid; i < FH_WIN_FLOATS; i += TR_BLOCK) s_win[i] = 0.0f;
    __syncthreads();
    const uint2 tile = tiles[blockIdx.x];
    const int x0 = (int)tile.x * 8, y0 = (int)tile.y * 8;
    const uint32_t px = (uint32_t)x0 + (lane & 7u), py = (uint32_t)y0 + (lane >> 3);
    const uint32_t kp = key_pixel(kf, py * sc.width + px);
    for (uint32_t s = smp_begin + wave; s < smp_end; s += TR_BLOCK / 64u) {   // (wave-uniform bounds)
        float sx, sy, t;
        pixel_sample(kp, s, spp, px, py, sx, sy, t);
        const FirstHit v = fh_sample<ANIM>(sc, scp, s_stack + tid, sx, sy, t, true);
        fh_splat(sc, s_win, s_table, x0, y0, sx, sy, v);
    }
    __syncthreads();
    const int wx0 = x0 - sc.fpw, wy0 = y0 - sc.fph;
    const int ww = 8 + 2 * sc.fpw + 1, wh = 8 + 2 * sc.fph + 1;
    for (int i = (int)tid; i < ww * wh; i += TR_BLOCK) {
        const int wy = i / ww, wx = i - wy * ww;
        const int ix = wx0 + wx, iy = wy0 + wy;
        if (ix < 0 || iy < 0 || ix >= (int)sc.width || iy >= (int)sc.height) continue;
        const int o = wy * WIN_STRIDE + wx;
        float v[FH_PLANES];
        bool any = false;
#pragma unroll
        for (int k = 0; k < FH_PLANES; ++k) { v[k] = s_win[o + k * WIN_PLANE]; any = any || v[k] != 0.0f; }
        if (!any) continue;   // (as the tile kernel skips an all-zero window pixel)
        const size_t p = ((size_t)iy * sc.width + ix) * 4;
        float* const films[3] = {albedo + p, normal + p, depth + p};
#pragma unroll
        for (int f = 0; f < 3; ++f) {
            atomicAdd(films[f] + 0, v[3 * f]);
            atomicAdd(films[f] + 1, v[3 * f + 1]);
            atomicAdd(films[f] + 2, v[3 * f + 2]);
            atomicAdd(films[f] + 3, v[9]);
        }
    }
}

// the per-sample statement for individual (px, py, s) items: twelve floats each (sx, sy, time, albedo, normal, t, hit, 0); the whole wave stays
// through the trace, as in k_debug_sample_radiance
template <int ANIM>
__global__ __launch_bounds__(TR_BLOCK) void k_debug_first_hit(const DevScene scv, uint32_t n, const uint32_t* __restrict__ px,
                                                              const uint32_t* __restrict__ py, const uint32_t* __restrict__ si, uint32_t spp,
                                                              uint32_t kf, float* __restrict__ out) {
    TR_DYN_LDS(uint32_t, s_stack);
    const DevScene& sc = scv;
    const DevScene* const scp = &scv;
    const uint32_t idx = blockIdx.x * blockDim.x + threadIdx.x;
    const bool in_range = idx < n;
    const uint32_t i = in_range ? idx : 0u;
    const uint32_t kp = key_pixel(kf, py[i] * sc.width + px[i]);
    float sx, sy, t;
    pixel_sample(kp, si[i], spp, px[i], py[i], sx, sy, t);
    const FirstHit v = fh_sample<ANIM>(sc, scp, s_stack + threadIdx.x, sx, sy, t, in_range);
    if (!in_range) return;
    float* const o = out + (size_t)i * 12;
    o[0] = sx; o[1] = sy; o[2] = t;
#pragma unroll
    for (int k = 0; k < 9; ++k) o[3 + k] = v.c[k];
}

// s(p) of tray_denoise_demodulated_device: max(ALB.rgb / ALB.w, 0) + TRAY_DEMOD_EPS where the albedo pixel is valid, else 1
TR_DEV bool fh_finite(float x) { return (__float_as_uint(x) & 0x7f800000u) != 0x7f800000u; }
TR_DEV f3 fh_scale(const float4 alb) {
    if (!(alb.w > 0.0f) || !fh_finite(alb.x) || !fh_finite(alb.y) || !fh_finite(alb.z) || !fh_finite(alb.w)) return mk(1.0f, 1.0f, 1.0f);
    return mk(fmaxf(alb.x / alb.w, 0.0f) + TRAY_DEMOD_EPS, fmaxf(alb.y / alb.w, 0.0f) + TRAY_DEMOD_EPS, fmaxf(alb.z / alb.w, 0.0f) + TRAY_DEMOD_EPS);
}
// E' = (E.rgb / s, E.w) and O' likewise, one thread per pixel
__global__ __launch_bounds__(TR_BLOCK) void k_fh_demodulate(const float4* __restrict__ even, const float4* __restrict__ odd, const float4* __restrict__ albedo,
                                                            uint32_t n_px, float4* __restrict__ even_out, float4* __restrict__ odd_out) {
    const uint32_t i = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (i >= n_px) return;
    const f3 s = fh_scale(albedo[i]);
    const float4 e = even[i], o = odd[i];
    even_out[i] = make_float4(e.x / s.x, e.y / s.y, e.z / s.z, e.w);
    odd_out[i] = make_float4(o.x / s.x, o.y / s.y, o.z / s.z, o.w);
}
// out = (D.rgb * s, 1) in place
__global__ __launch_bounds__(TR_BLOCK) void k_fh_remodulate(const float4* __restrict__ albedo, uint32_t n_px, float4* __restrict__ out) {
    const uint32_t i = blockIdx.x * TR_BLOCK + threadIdx.x;
    if (i >= n_px) return;
    const f3 s = fh_scale(albedo[i]);
    const float4 d = out[i];
    out[i] = make_float4(d.x * s.x, d.y * s.y, d.z * s.z, 1.0f);
}
