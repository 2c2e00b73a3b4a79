// The second pass over all frames of tray_denoise_temporal_halves_device / _guided_device / _two_pass_device (include/trayhip.h):
// k_t2p_halves_pass and k_t2p_guided_pass (t2pass_kernels.h) live in libtrayhip_t2pass.so, compiled from t2pass.hip; device_api.hip launches
// them through these functions, between tr_denoise::prepare's and tr_guide::halves' launches (denoise.h, guide.h), so that libtrayhip.so's and
// every other add-on library's code objects stay what they were.
#pragma once
#include "denoise.h"

namespace tr_t2pass {
// launches of one call with N neighbours. Halves: per frame prepare's two and one k_t2p_halves_pass. Guided: per frame prepare of the values,
// prepare of the guide, one k_t2p_guided_pass. Two-pass: the halves call; prepare of the centre's pilot and the centre's guided pass; per
// neighbour prepare of its films, k_dn_filter_halves, prepare of its pilot, its guided pass.
constexpr uint32_t halves_launches(uint32_t n) { return (tr_denoise::kPrepareLaunches + 1u) * (n + 1u); }
constexpr uint32_t guided_launches(uint32_t n) { return (2u * tr_denoise::kPrepareLaunches + 1u) * (n + 1u); }
constexpr uint32_t two_pass_launches(uint32_t n) { return halves_launches(n) + tr_denoise::kPrepareLaunches + 1u + (2u * tr_denoise::kPrepareLaunches + 2u) * n; }
// bytes of scratch of the three calls for a width x height film, whatever N is, and their regions (t2pass_kernels.h has the layouts)
uint64_t halves_scratch_bytes(uint32_t width, uint32_t height);   // 128 per pixel: tr_temporal::scratch_bytes
struct HalvesLayout { void* centre; void* neighbour; void* sums; };
HalvesLayout halves_layout(void* scratch, uint32_t width, uint32_t height);
uint64_t guided_scratch_bytes(uint32_t width, uint32_t height);   // 176 per pixel
struct GuidedLayout { void* centre_guide; void* guide; void* values; void* sums; };
GuidedLayout guided_layout(void* scratch, uint32_t width, uint32_t height);
uint64_t two_pass_scratch_bytes(uint32_t width, uint32_t height);   // 256 per pixel
struct TwoPassLayout { void* centre; void* neighbour; void* sums; float* fa; float* fb; void* centre_guide; void* guide; };
TwoPassLayout two_pass_layout(void* scratch, uint32_t width, uint32_t height);
// one k_t2p_halves_pass<patch> over all 32 x 16 tiles, as tr_temporal::pass; last: the normalised halves go to fa / fb
void halves_pass(hipStream_t stream, const void* centre_records, const void* frame_records, uint32_t width, uint32_t height, uint32_t radius, uint32_t patch,
                 float k, void* sums, bool first, bool last, float* fa, float* fb);
// one k_t2p_guided_pass<patch> over all 32 x 16 tiles: weights between the patches of centre_guide_records and the window of guide_records, applied
// to the colours of value_records (tr_denoise::prepare's, all three), added to the sums (first: they start at 0); last: the normalised image goes to out
void guided_pass(hipStream_t stream, const void* centre_guide_records, const void* guide_records, const void* value_records, uint32_t width, uint32_t height,
                 uint32_t radius, uint32_t patch, float k, void* sums, bool first, bool last, float* out);
}  // namespace tr_t2pass
