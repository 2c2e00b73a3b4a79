// The two-pass temporal filter on albedo-demodulated films of tray_denoise_temporal_demodulated_halves_device / _guided_device / _two_pass_device
// (include/trayhip.h): k_td2_guided_pass and instances of k_tdm_prepare and k_dn_prepare<1> (td2pass_kernels.h) live in libtrayhip_td2pass.so,
// compiled from td2pass.hip; device_api.hip launches them through these functions, between tr_denoise::prepare's, tr_guide::halves' and
// tr_t2pass::halves_pass' launches (denoise.h, guide.h, t2pass.h), so that libtrayhip.so's and every other add-on library's code objects stay
// what they were. The three calls' schedules, launch counts and scratch layouts -- the two-pass temporal calls' -- are denoise_plan.h's.
#pragma once

namespace tr_td2pass {
// the two preparing launches of one frame's values: k_tdm_prepare (the records of the films divided by the scale of `albedo`), then k_dn_prepare<1>
void prepare(hipStream_t stream, const float* even, const float* odd, const float* albedo, uint32_t width, uint32_t height, void* records);
// one k_td2_guided_pass<patch> over all 32 x 16 tiles, as tr_t2pass::guided_pass; last: the normalised image times the scale of `albedo` (the
// centre frame's) goes to out
void guided_pass(hipStream_t stream, const void* centre_guide_records, const void* guide_records, const void* value_records, const float* albedo,
                 uint32_t width, uint32_t height, uint32_t radius, uint32_t patch, float k, void* sums, bool first, bool last, float* out);
}  // namespace tr_td2pass
