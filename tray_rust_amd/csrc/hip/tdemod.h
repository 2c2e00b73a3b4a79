// The albedo-demodulated temporal filter of tray_denoise_temporal_demodulated_device (include/trayhip.h): k_tdm_prepare, k_tdm_pass and an instance
// of k_dn_prepare<1> (tdemod_kernels.h) live in libtrayhip_tdemod.so, compiled from tdemod.hip; device_api.hip launches them through these
// functions, so that libtrayhip.so's and every other add-on library's code objects stay what they were. The call's schedule and scratch layout (the
// temporal call's) are denoise_plan.h's.
#pragma once

namespace tr_tdemod {
// the two preparing launches of one frame: k_tdm_prepare (the records of the films divided by the scale of `albedo`), then k_dn_prepare<1>
void prepare(hipStream_t stream, const float* even, const float* odd, const float* albedo, uint32_t width, uint32_t height, void* records);
// one k_tdm_pass<patch> over all 32 x 16 tiles, as tr_temporal::pass; last: the normalised image times the scale of `albedo` (the centre frame's)
// goes to out
void pass(hipStream_t stream, const void* centre_records, const void* frame_records, const float* albedo, uint32_t width, uint32_t height, uint32_t radius,
          uint32_t patch, float k, void* sums, bool first, bool last, float* out);
}  // namespace tr_tdemod
