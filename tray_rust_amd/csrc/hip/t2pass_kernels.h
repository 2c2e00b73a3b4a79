// The kernels of tray_denoise_temporal_halves_device, tray_denoise_temporal_guided_device and tray_denoise_temporal_two_pass_device
// (include/trayhip.h states them): the temporal filter of temporal_kernels.h with the two ends it lacks for a second pass over all frames.
// k_t2p_halves_pass is k_tdn_pass whose last pass stores the two cross-filtered halves as films of their own (the pilot of the centre frame over
// all frames' windows); k_t2p_guided_pass is k_tdn_pass whose weights are measured on the frames' GUIDES and applied to the frames' VALUES.
// Every frame is resolved by the unchanged k_dn_prepare<0> / <1> of libtrayhip_denoise.so into records of its own. Device code only; compiled
// into libtrayhip_t2pass.so by t2pass.hip, and by g++ into the host emulation (tests/emu/emu_temporal2.cpp). All arithmetic is f32 and
// unfused (-ffp-contract=off).
//
// Scratch buffers, n = width * height float4 records each, whatever N is (the neighbours are processed one at a time):
//   halves call (t2p_halves_scratch_bytes = 128 bytes per pixel): temporal_kernels.h's, region for region
//     [0, 3 n)     A4, B4, V4 of the centre frame
//     [3 n, 6 n)   A4, B4, V4 of the neighbour of the current pass
//     [6 n, 8 n)   the sums between passes
//   guided call (t2p_guided_scratch_bytes = 176 bytes per pixel)
//     [0, 3 n)     the records of the centre's guide (guide_a, guide_b)
//     [3 n, 6 n)   the records of the guide of the neighbour of the current pass
//     [6 n, 9 n)   the records of the VALUES of the frame of the current pass (V4 is written and not read)
//     [9 n, 11 n)  the sums between passes
//   two-pass call (t2p_two_pass_scratch_bytes = 256 bytes per pixel)
//     [0, 3 n)     the records of the centre's films: the first pass's centre and the second pass's values of frame 0
//     [3 n, 6 n)   the records of the current neighbour's films: the first pass's neighbour, the neighbour's own pilot's input and the second
//                  pass's values of that frame
//     [6 n, 8 n)   the sums between passes, of the first pass and then of the second
//     [8 n, 10 n)  fa, fb: the pilot of the frame in hand as RGBW films (the centre's over all frames, then each neighbour's own)
//     [10 n, 13 n) the records of the centre's pilot
//     [13 n, 16 n) the records of the current neighbour's pilot
//
// Both kernels are a front and an end around dn_filter_block<F, DN_P_CENTRE, QV> (denoise_kernels.h, "Two sources"), called by every thread
// unconditionally, with no store before its last barrier:
//   k_t2p_halves_pass   QV = DN_Q_STAGED: the pass's frame is staged, p' of step 1 comes from the centre's records. The last pass stores
//                       fa = (A, wA) and fb = (B, wB) as k_dn_filter_halves does, two float4 stores per thread; every other pass stores the sums.
//                       (fa.rgb + fb.rgb) * 0.5f is k_tdn_pass's out.rgb, being dn_mean of the same dn_normalise of the same sums.
//   k_t2p_guided_pass   QV = DN_Q_GLOBAL: the pass's frame's GUIDE records are staged, p' of step 1 comes from the centre's GUIDE records, and
//                       a(q), b(q), valid(q) of step 3 are two float4 loads per thread and offset from the pass's frame's VALUE records, issued
//                       at the top of the offset's iteration, so that steps 1 and 2 and both barriers stand between the loads and their use. A
//                       half wave reads 32 consecutive records of one row (512 contiguous bytes per array). The end is k_tdn_pass's.
// The sums are carried in `acc` exactly as k_tdn_pass carries them: a thread reads and writes its own pixel's words only, no atomics, every word
// written once per pass, the same bits in every run. With the guides' records as the values' the guided pass is k_tdn_pass operation for
// operation (a(q), b(q), valid(q) are the same words from another address space); with one frame it is k_gdn_filter (guided_kernels.h).
#pragma once
#include "denoise_kernels.h"

namespace tr_t2pass {

using namespace tr_denoise;

__host__ __device__ inline uint64_t t2p_halves_scratch_bytes(uint32_t width, uint32_t height) { return (uint64_t)width * height * 128u; }
__host__ __device__ inline uint64_t t2p_guided_scratch_bytes(uint32_t width, uint32_t height) { return (uint64_t)width * height * 176u; }
__host__ __device__ inline uint64_t t2p_two_pass_scratch_bytes(uint32_t width, uint32_t height) { return (uint64_t)width * height * 256u; }

// the end both kernels share with k_tdn_pass: every pass but the last stores the sums back (after dn_filter_block's last barrier, inside the image)
TR_DEV void t2p_store_sums(const dn_sums& s, size_t p, size_t n, float4* __restrict__ acc) {
    acc[p] = s.A;
    acc[n + p] = s.B;
}

// one pass of the pilot: the window of `frame` (records of k_dn_prepare, 3 n float4) around every pixel, with the patches of `centre` (likewise;
// the same buffer in the centre's own pass) on the p side; acc: 2 n float4; fa, fb: n float4 each, written when last != 0
template <int F>
__global__ __launch_bounds__(DN_BLOCK) void k_t2p_halves_pass(const float4* __restrict__ centre, const float4* __restrict__ frame, uint32_t width,
                                                              uint32_t height, uint32_t radius, float k, float4* __restrict__ acc, uint32_t first,
                                                              uint32_t last, float4* __restrict__ fa, float4* __restrict__ fb) {
    const dn_sums s = dn_filter_block<F, DN_P_CENTRE, DN_Q_STAGED>(frame, centre, nullptr, width, height, radius, k, blockIdx.x, first == 0u ? acc : nullptr);
    if (s.px >= width || s.py >= height) return;   // (after the last barrier)
    const size_t p = (size_t)s.py * width + s.px;
    if (last != 0u) {
        const dn_halves h = dn_normalise(s);
        fa[p] = h.A;
        fb[p] = h.B;
    } else {
        t2p_store_sums(s, p, (size_t)width * height, acc);
    }
}

// one pass of the second filter: the window of one frame around every pixel. centre_guide, guide: the records of the centre's and of the pass's
// frame's guide (3 n float4 each; the same buffer in the centre's own pass); values: the records of the pass's frame's values (of which A4 and
// B4 are read); acc: 2 n float4; out: n float4, written when last != 0
template <int F>
__global__ __launch_bounds__(DN_BLOCK) void k_t2p_guided_pass(const float4* __restrict__ centre_guide, const float4* __restrict__ guide,
                                                              const float4* __restrict__ values, uint32_t width, uint32_t height, uint32_t radius, float k,
                                                              float4* __restrict__ acc, uint32_t first, uint32_t last, float4* __restrict__ out) {
    const dn_sums s = dn_filter_block<F, DN_P_CENTRE, DN_Q_GLOBAL>(guide, centre_guide, values, width, height, radius, k, blockIdx.x, first == 0u ? acc : nullptr);
    if (s.px >= width || s.py >= height) return;   // (after the last barrier)
    const size_t p = (size_t)s.py * width + s.px;
    if (last != 0u) out[p] = dn_mean(dn_normalise(s));
    else t2p_store_sums(s, p, (size_t)width * height, acc);
}

}  // namespace tr_t2pass
