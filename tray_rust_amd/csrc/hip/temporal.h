// The temporal filter of tray_denoise_temporal_device (include/trayhip.h): k_tdn_pass (temporal_kernels.h) lives in libtrayhip_temporal.so, compiled
// from temporal.hip; device_api.hip launches it through these functions, between tr_denoise::prepare's launches (denoise.h), so that
// libtrayhip.so's own code objects stay what they were. The call's schedule and scratch layout are denoise_plan.h's.
#pragma once

namespace tr_temporal {
// one k_tdn_pass<patch> over all 32 x 16 tiles: the window of radius `radius` of `frame_records` (tr_denoise::prepare's) around every pixel, with the
// patches of `centre_records` on the other side, added to the sums (first: they start at 0); last: the normalised image goes to out
void pass(hipStream_t stream, const void* centre_records, const void* frame_records, uint32_t width, uint32_t height, uint32_t radius, uint32_t patch, float k,
          void* sums, bool first, bool last, float* out);
}  // namespace tr_temporal
