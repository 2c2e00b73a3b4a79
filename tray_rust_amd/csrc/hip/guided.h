// The guided filter of tray_denoise_guided_device / tray_denoise_two_pass_device (include/trayhip.h): k_gdn_filter (guided_kernels.h) lives in
// libtrayhip_guided.so, compiled from guided.hip; device_api.hip launches it through these functions, after tr_denoise::prepare's launches
// (denoise.h) for the values and for the guide, so that libtrayhip.so's own code objects stay what they were.
#pragma once
#include "denoise.h"

namespace tr_guided {
// launches of one tray_denoise_guided_device call: tr_denoise::prepare of the values, of the guide, k_gdn_filter<patch>
constexpr uint32_t kLaunches = 2u * tr_denoise::kPrepareLaunches + 1u;
// ... and of one tray_denoise_two_pass_device call: prepare of the films, k_dn_filter_halves<patch>, prepare of the pilot, k_gdn_filter<patch2>
constexpr uint32_t kTwoPassLaunches = 2u * tr_denoise::kPrepareLaunches + 2u;
// bytes of scratch of a guided call for a width x height film: the values' records and the guide's (96 per pixel)
uint64_t scratch_bytes(uint32_t width, uint32_t height);
struct Layout { void* values; void* guide; };
Layout layout(void* scratch, uint32_t width, uint32_t height);
// bytes of scratch of a two-pass call: the films' records (the first pass's scratch and the second pass's values), the pilot fa / fb, and the
// pilot's records (128 per pixel)
uint64_t two_pass_scratch_bytes(uint32_t width, uint32_t height);
struct TwoPassLayout { void* values; float* fa; float* fb; void* guide; };
TwoPassLayout two_pass_layout(void* scratch, uint32_t width, uint32_t height);
// one k_gdn_filter<patch> over all 32 x 16 tiles: weights from guide_records, colours and validity from value_records (tr_denoise::prepare's, both)
void filter(hipStream_t stream, const void* guide_records, const void* value_records, uint32_t width, uint32_t height, uint32_t radius, uint32_t patch, float k,
            float* out);
}  // namespace tr_guided
