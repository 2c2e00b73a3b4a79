// The filtered halves and the block lists of tray_denoise_halves_device / tray_render_noise_target_filtered_device (include/trayhip.h):
// k_dn_filter_halves, k_guide_mark and k_guide_compact (guide_kernels.h) live in libtrayhip_guide.so, compiled from guide.hip; device_api.hip
// launches them through these functions, so that libtrayhip.so's own code objects stay what they were.
#pragma once

namespace tr_guide {
// 32 x 16 pixel blocks of a width x height frame (k_dn_filter's tiles; guide.hip checks the two constants against the kernels')
constexpr uint32_t kBlockW = 32u, kBlockH = 16u;
uint32_t blocks_x(uint32_t width);
uint32_t blocks_y(uint32_t height);
// fa / fb = the cross-filtered halves of the prepared scratch (tr_denoise::prepare), over the n_blocks blocks of `blocks`, or over every block
// when blocks is null; n_blocks == 0 with a list launches nothing. Returns the number of launches (0 or 1).
uint32_t halves(hipStream_t stream, const void* scratch, uint32_t width, uint32_t height, uint32_t radius, uint32_t patch, float k, const uint32_t* blocks,
                uint32_t n_blocks, float* fa, float* fb);
// flags[block] = 1 for every block that holds a tile of queue[0, n) whose active word is set (active == null: every tile)
void mark(hipStream_t stream, const uint2* queue, const uint32_t* active, uint32_t n, uint32_t width, uint32_t height, uint32_t* flags);
// the set flags' block indices in rising order into list, their number into *count
void compact(hipStream_t stream, const uint32_t* flags, uint32_t width, uint32_t height, uint32_t* list, uint32_t* count);
}  // namespace tr_guide
