// The kernels of tray_denoise_temporal_demodulated_device (include/trayhip.h states it): the temporal filter of temporal_kernels.h on films that are
// divided by their own frame's first-hit albedo on the way in, with the centre frame's albedo multiplied back in on the way out. By definition the
// call is k_fh_demodulate (first_hit_kernels.h) of every frame, tray_denoise_temporal_device of the quotients, k_fh_remodulate of its output; the
// two element-wise steps are folded into the filter's first and last launch here, so that no E' / O' film is written to memory and the call
// stays 3 (N + 1) launches over the temporal call's 128 bytes of scratch per pixel. Device code only; compiled into libtrayhip_tdemod.so by
// tdemod.hip, and by g++ into the host emulation (tests/emu/emu_tdemod.cpp). All arithmetic is f32 and unfused (-ffp-contract=off).
//
// Per frame: k_tdm_prepare (the A4 / B4 records of the demodulated films), the unchanged k_dn_prepare<1> (V4 from those records; this library
// holds an instance of its own), k_tdm_pass (one frame's window added to the eight sums). The scratch buffer is temporal_kernels.h's, region for
// region.
//
// tdm_scale restates fh_scale (first_hit_kernels.h), which lives behind the render kernels' headers, and the first half of k_tdm_prepare restates
// k_fh_demodulate, the second k_dn_prepare<0>: operation for operation, in their order. tests/test_tdemod_emu.py holds the copies together: with
// N = 0 the call gives tray_denoise_demodulated_device's bits on albedo films with invalid, zero and negative pixels, and in general the bits of
// the three separate steps.
#pragma once
#include "../../../include/trayhip.h"   // TRAY_DEMOD_EPS
#include "denoise_kernels.h"

namespace tr_tdemod {

using namespace tr_denoise;

__host__ __device__ inline uint64_t tdm_scratch_bytes(uint32_t width, uint32_t height) { return (uint64_t)width * height * 128u; }

// s(p) of tray_denoise_demodulated_device: max(ALB.rgb / ALB.w, 0) + TRAY_DEMOD_EPS where the albedo pixel is valid, else 1
struct tdm_s3 { float x, y, z; };
TR_DEV tdm_s3 tdm_scale(const float4 alb) {
    if (!(alb.w > 0.0f) || !dn_finite(alb.x) || !dn_finite(alb.y) || !dn_finite(alb.z) || !dn_finite(alb.w)) return tdm_s3{1.0f, 1.0f, 1.0f};
    return tdm_s3{fmaxf(alb.x / alb.w, 0.0f) + TRAY_DEMOD_EPS, fmaxf(alb.y / alb.w, 0.0f) + TRAY_DEMOD_EPS, fmaxf(alb.z / alb.w, 0.0f) + TRAY_DEMOD_EPS};
}

// k_fh_demodulate followed by k_dn_prepare<0> in one pass: E' = (E.rgb / s, E.w), O' likewise, held in registers; then A4 and B4 of (E', O'),
// whose validity is tested on the quotients' words. One thread per pixel, three float4 loads, two float4 stores; two divisions per channel,
// / s then / w.
__global__ __launch_bounds__(DN_PREP_BLOCK) void k_tdm_prepare(const float4* __restrict__ even, const float4* __restrict__ odd, const float4* __restrict__ albedo,
                                                               uint32_t width, uint32_t height, float4* __restrict__ scratch) {
    const size_t n = (size_t)width * height;
    const size_t p = (size_t)blockIdx.x * DN_PREP_BLOCK + threadIdx.x;
    if (p >= n) return;
    float4* const A4 = scratch;
    float4* const B4 = scratch + n;
    const tdm_s3 s = tdm_scale(albedo[p]);
    const float4 e = even[p], o = odd[p];
    const float4 E = make_float4(e.x / s.x, e.y / s.y, e.z / s.z, e.w);
    const float4 O = make_float4(o.x / s.x, o.y / s.y, o.z / s.z, o.w);
    const bool valid = E.w > 0.0f && O.w > 0.0f && dn_finite4(E) && dn_finite4(O);
    float4 a = make_float4(0.0f, 0.0f, 0.0f, 0.0f), b = a;
    if (valid) {
        a = make_float4(E.x / E.w, E.y / E.w, E.z / E.w, 1.0f);
        b = make_float4(O.x / O.w, O.y / O.w, O.z / O.w, 0.0f);
    }
    A4[p] = a;
    B4[p] = b;
}

// k_tdn_pass (temporal_kernels.h) with k_fh_remodulate folded into the last pass's store: out = (D.rgb * s_0, 1) with s_0 from the centre frame's
// albedo pixel, loaded after dn_filter_block's last barrier by the threads inside the image. Every other pass stores the sums, as k_tdn_pass.
template <int F>
__global__ __launch_bounds__(DN_BLOCK) void k_tdm_pass(const float4* __restrict__ centre, const float4* __restrict__ frame, const float4* __restrict__ albedo,
                                                       uint32_t width, uint32_t height, uint32_t radius, float k, float4* __restrict__ acc, uint32_t first,
                                                       uint32_t last, float4* __restrict__ out) {
    const dn_sums s = dn_filter_block<F, DN_P_CENTRE>(frame, centre, nullptr, width, height, radius, k, blockIdx.x, first == 0u ? acc : nullptr);
    if (s.px >= width || s.py >= height) return;   // (after the last barrier)
    const size_t p = (size_t)s.py * width + s.px;
    if (last != 0u) {
        const float4 d = dn_mean(dn_normalise(s));
        const tdm_s3 sc = tdm_scale(albedo[p]);
        out[p] = make_float4(d.x * sc.x, d.y * sc.y, d.z * sc.z, 1.0f);
    } else {
        acc[p] = s.A;
        acc[(size_t)width * height + p] = s.B;
    }
}

}  // namespace tr_tdemod
