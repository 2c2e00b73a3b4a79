// The per-round epilogue of tray_render_noise_target_device (include/trayhip.h): k_noise_error and k_noise_compact (noise_kernels.h) live in
// libtrayhip_noise.so, compiled from noise.hip; device_api.hip launches them through these functions, so that libtrayhip.so's own code objects stay
// what they were.
#pragma once

namespace tr_noise {
// the error, samples and next-round flag of the n_active tiles of `tiles` (queue indices qidx, or 0 .. n_active - 1 when qidx is null)
void error(hipStream_t stream, const float* even, const float* odd, uint32_t width, uint32_t height, const uint2* tiles, const uint32_t* qidx,
           uint32_t n_active, uint32_t n_taken, uint32_t max_spp, float threshold, float* err, uint32_t* active, uint32_t* samples);
// the flagged tiles of queue[0, n) in queue order into out_tiles / out_q, their number into *count
void compact(hipStream_t stream, const uint2* queue, const uint32_t* active, uint32_t n, uint2* out_tiles, uint32_t* out_q, uint32_t* count);
}  // namespace tr_noise
