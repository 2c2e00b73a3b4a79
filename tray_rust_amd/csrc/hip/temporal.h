// The temporal filter of tray_denoise_temporal_device (include/trayhip.h): k_tdn_pass (temporal_kernels.h) lives in libtrayhip_temporal.so, compiled
// from temporal.hip; device_api.hip launches it through these functions, between tr_denoise::prepare's launches (denoise.h), so that
// libtrayhip.so's own code objects stay what they were.
#pragma once

namespace tr_temporal {
// bytes of scratch of a call for a width x height film: the centre's records, one neighbour's records and the sums (128 per pixel)
uint64_t scratch_bytes(uint32_t width, uint32_t height);
// the three regions of that buffer
struct Layout { void* centre; void* neighbour; void* sums; };
Layout layout(void* scratch, uint32_t width, uint32_t height);
// one k_tdn_pass<patch> over all 32 x 16 tiles: the window of radius `radius` of `frame_records` (tr_denoise::prepare's) around every pixel, with the
// patches of `centre_records` on the other side, added to the sums (first: they start at 0); last: the normalised image goes to out
void pass(hipStream_t stream, const void* centre_records, const void* frame_records, uint32_t width, uint32_t height, uint32_t radius, uint32_t patch, float k,
          void* sums, bool first, bool last, float* out);
}  // namespace tr_temporal
