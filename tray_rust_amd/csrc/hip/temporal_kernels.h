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
// k_tdn_pass is dn_filter_block<F, DN_P_CENTRE> (denoise_kernels.h, "Two sources") between a front and an end: the PASS'S frame is staged, p' of
// step 1 comes from the CENTRE frame's records, a(q), b(q) and valid(q) of step 3 are the pass's frame's, and the eight sums start at 0 (first) or
// at what `acc` holds. The last pass stores the normalised ((A + B) / 2, 1) into `out`, every other pass stores the sums back. A thread reads and
// writes its own pixel's words only: no atomics, every word written once per pass, the same bits in every run. With the centre as the pass's
// frame, first = last = 1, every operation and its order are k_dn_filter's, being the same function: the same bits.
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
    const dn_sums s = dn_filter_block<F, DN_P_CENTRE>(frame, centre, nullptr, width, height, radius, k, blockIdx.x, first == 0u ? acc : nullptr);
    if (s.px >= width || s.py >= height) return;   // (after the last barrier)
    const size_t p = (size_t)s.py * width + s.px;
    if (last != 0u) {
        out[p] = dn_mean(dn_normalise(s));
    } else {
        acc[p] = s.A;
        acc[(size_t)width * height + p] = s.B;
    }
}

}  // namespace tr_temporal
