// The guided filter of tray_denoise_guided_device / tray_denoise_two_pass_device (include/trayhip.h): k_gdn_filter (guided_kernels.h) lives in
// libtrayhip_guided.so, compiled from guided.hip; device_api.hip launches it through these functions, after tr_denoise::prepare's launches
// (denoise.h) for the values and for the guide, so that libtrayhip.so's own code objects stay what they were. The two calls' schedules, launch
// counts and scratch layouts are denoise_plan.h's.
#pragma once

namespace tr_guided {
// one k_gdn_filter<patch> over all 32 x 16 tiles: weights from guide_records, colours and validity from value_records (tr_denoise::prepare's, both)
void filter(hipStream_t stream, const void* guide_records, const void* value_records, uint32_t width, uint32_t height, uint32_t radius, uint32_t patch, float k,
            float* out);
}  // namespace tr_guided
