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
// k_gdn_filter is dn_filter_block<F, DN_P_STAGED, DN_Q_GLOBAL> (denoise_kernels.h, "Two sources") and k_dn_filter's end: the GUIDE'S records are
// staged and measured, and a(q), b(q) and valid(q) of step 3 are the VALUES': two float4 loads per thread and offset from the values' records in
// global memory. A half wave reads 32 consecutive records of one row (512 contiguous bytes per array); the tile's window of values is
// (32 + 2r) x (16 + 2r) x 32 bytes (35 KB at r = 5) and stays in the CU's vector cache and in L2 after the first offsets.
// Why not LDS: at r = 10, f = 3 the values' window beside the guide's region comes to 161 082 of gfx950's 163 840 bytes only with a validity
// bitmask and three float2 arrays of another layout than the guide's, i.e. a second staging loop and a second set of bank rules for 1.7 % of
// head room; one workgroup per CU fits either way, so LDS residency would buy no occupancy, only the latency that the early loads already hide.
// With the guide's records as the values' (the same films twice), every operation and its order are k_dn_filter's, being the same function: the
// same bits.
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
    const dn_sums s = dn_filter_block<F, DN_P_STAGED, DN_Q_GLOBAL>(guide, nullptr, values, width, height, radius, k, blockIdx.x, nullptr);
    if (s.px < width && s.py < height) out[(size_t)s.py * width + s.px] = dn_mean(dn_normalise(s));
}

}  // namespace tr_guided
