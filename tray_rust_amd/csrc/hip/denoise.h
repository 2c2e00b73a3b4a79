// The filter of tray_denoise_device (include/trayhip.h): k_dn_prepare and k_dn_filter (denoise_kernels.h) live in libtrayhip_denoise.so, compiled
// from denoise.hip; device_api.hip launches them through these functions, so that libtrayhip.so's own code objects stay what they were.
#pragma once

namespace tr_denoise {
// launches of one denoise(): k_dn_prepare<0>, k_dn_prepare<1>, k_dn_filter<patch>
constexpr uint32_t kLaunches = 3u;
// the first two launches of denoise(): k_dn_prepare<0> and <1> resolve the films into the scratch records that k_dn_filter and k_dn_filter_halves read
constexpr uint32_t kPrepareLaunches = 2u;
void prepare(hipStream_t stream, const float* even, const float* odd, uint32_t width, uint32_t height, void* scratch);
// out = the filter of even / odd (width * height RGBW pixels each, 16-byte aligned like scratch); 1 <= radius <= 10, patch <= 3, width, height >= 1
void denoise(hipStream_t stream, const float* even, const float* odd, uint32_t width, uint32_t height, uint32_t radius, uint32_t patch, float k, float* out,
             void* scratch);
}  // namespace tr_denoise
