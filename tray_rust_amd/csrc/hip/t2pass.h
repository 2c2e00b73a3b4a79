// The second pass over all frames of tray_denoise_temporal_halves_device / _guided_device / _two_pass_device (include/trayhip.h):
// k_t2p_halves_pass and k_t2p_guided_pass (t2pass_kernels.h) live in libtrayhip_t2pass.so, compiled from t2pass.hip; device_api.hip launches
// them through these functions, between tr_denoise::prepare's and tr_guide::halves' launches (denoise.h, guide.h), so that libtrayhip.so's and
// every other add-on library's code objects stay what they were. The three calls' schedules, launch counts and scratch layouts are denoise_plan.h's
// (t2pass_kernels.h documents the layouts).
#pragma once

namespace tr_t2pass {
// one k_t2p_halves_pass<patch> over all 32 x 16 tiles, as tr_temporal::pass; last: the normalised halves go to fa / fb
void halves_pass(hipStream_t stream, const void* centre_records, const void* frame_records, uint32_t width, uint32_t height, uint32_t radius, uint32_t patch,
                 float k, void* sums, bool first, bool last, float* fa, float* fb);
// one k_t2p_guided_pass<patch> over all 32 x 16 tiles: weights between the patches of centre_guide_records and the window of guide_records, applied
// to the colours of value_records (tr_denoise::prepare's, all three), added to the sums (first: they start at 0); last: the normalised image goes to out
void guided_pass(hipStream_t stream, const void* centre_guide_records, const void* guide_records, const void* value_records, uint32_t width, uint32_t height,
                 uint32_t radius, uint32_t patch, float k, void* sums, bool first, bool last, float* out);
}  // namespace tr_t2pass
