// The kernels of tray_denoise_temporal_demodulated_halves_device, tray_denoise_temporal_demodulated_guided_device and
// tray_denoise_temporal_demodulated_two_pass_device (include/trayhip.h states them): the two-pass temporal filter of t2pass_kernels.h on films
// that are divided by their own frame's first-hit albedo on the way in, with the centre frame's albedo multiplied back in on the way out. By
// definition the two-pass call is k_fh_demodulate (first_hit_kernels.h) of every frame, tray_denoise_temporal_two_pass_device of the quotients,
// k_fh_remodulate of its output; both element-wise steps are folded into launches the two-pass temporal call makes anyway, so that no E' / O'
// film is written to memory and the calls keep that call's launch counts and scratch layouts (t2pass_kernels.h, region for region: 128 / 176 /
// 256 bytes per pixel). Device code only; compiled into libtrayhip_td2pass.so by td2pass.hip, and by g++ into the host emulation
// (tests/emu/emu_td2pass.cpp). All arithmetic is f32 and unfused (-ffp-contract=off).
//
// Where the two steps go:
//   in    every frame's VALUE records come from k_tdm_prepare (tdemod_kernels.h: demodulate and resolve in one pass) followed by the unchanged
//         k_dn_prepare<1>, where the two-pass temporal call has k_dn_prepare<0> and <1>; this library holds an instance of each. The records
//         are all the filter reads of a frame's films, so everything behind them works in the demodulated domain: the first pass
//         (k_t2p_halves_pass), a neighbour's own pilot (k_dn_filter_halves) and the pilots' records (k_dn_prepare<0> / <1>: the pilots ARE
//         demodulated films, resolved as they are) are launched from the libraries that hold them, unchanged.
//   out   k_td2_guided_pass: k_t2p_guided_pass whose last pass stores dn_mean(dn_normalise(s)) * tdm_scale(albedo_0[p]) with weight 1 -- the end
//         of k_tdm_pass on the body of k_t2p_guided_pass. The halves call has no way out: fa and fb are guides and stay demodulated.
//
// k_td2_guided_pass is a front and an end around dn_filter_block<F, DN_P_CENTRE, DN_Q_GLOBAL> (denoise_kernels.h, "Two sources"): every thread
// of the workgroup calls the body unconditionally, there is no store before its last barrier, and a thread outside the image returns after it
// without a store. The centre's albedo pixel is loaded after that barrier by the threads inside the image, in the last pass only. The sums are
// carried in `acc` as k_t2p_guided_pass carries them (t2p_store_sums): a thread reads and writes its own pixel's words only.
#pragma once
#include "tdemod_kernels.h"
#include "t2pass_kernels.h"

namespace tr_td2pass {

using namespace tr_denoise;
using tr_tdemod::k_tdm_prepare;
using tr_tdemod::tdm_s3;
using tr_tdemod::tdm_scale;

__host__ __device__ inline uint64_t td2_halves_scratch_bytes(uint32_t width, uint32_t height) { return tr_t2pass::t2p_halves_scratch_bytes(width, height); }
__host__ __device__ inline uint64_t td2_guided_scratch_bytes(uint32_t width, uint32_t height) { return tr_t2pass::t2p_guided_scratch_bytes(width, height); }
__host__ __device__ inline uint64_t td2_two_pass_scratch_bytes(uint32_t width, uint32_t height) { return tr_t2pass::t2p_two_pass_scratch_bytes(width, height); }

// one pass of the second filter, as k_t2p_guided_pass: centre_guide, guide: the records of the centre's and of the pass's frame's guide (3 n
// float4 each; the same buffer in the centre's own pass); values: the records of the pass's frame's demodulated values; albedo: the centre
// frame's albedo film (n float4, read when last != 0); acc: 2 n float4; out: n float4, written when last != 0
template <int F>
__global__ __launch_bounds__(DN_BLOCK) void k_td2_guided_pass(const float4* __restrict__ centre_guide, const float4* __restrict__ guide,
                                                              const float4* __restrict__ values, const float4* __restrict__ albedo, uint32_t width,
                                                              uint32_t height, uint32_t radius, float k, float4* __restrict__ acc, uint32_t first,
                                                              uint32_t last, float4* __restrict__ out) {
    const dn_sums s = dn_filter_block<F, DN_P_CENTRE, DN_Q_GLOBAL>(guide, centre_guide, values, width, height, radius, k, blockIdx.x, first == 0u ? acc : nullptr);
    if (s.px >= width || s.py >= height) return;   // (after the last barrier)
    const size_t p = (size_t)s.py * width + s.px;
    if (last != 0u) {
        const float4 d = dn_mean(dn_normalise(s));
        const tdm_s3 sc = tdm_scale(albedo[p]);
        out[p] = make_float4(d.x * sc.x, d.y * sc.y, d.z * sc.z, 1.0f);
    } else {
        tr_t2pass::t2p_store_sums(s, p, (size_t)width * height, acc);
    }
}

}  // namespace tr_td2pass
