// The neighbour bound of the two noise-target calls (include/trayhip.h: tray_scene_set_noise_ratio): k_nb_grid, k_nb_pull and k_nb_compact_level
// (nbound_kernels.h) live in libtrayhip_nbound.so, compiled from nbound.hip; device_api.hip launches them through these functions, so that the
// other libraries' code objects stay what they were.
#pragma once

namespace tr_nbound {
// map[0, grid_w * grid_h) = 0xffffffff (a memset on the stream), then the queue index of every tile of queue[0, n) at its cell: one launch
hipError_t grid(hipStream_t stream, const uint2* queue, uint32_t n, uint32_t grid_w, uint32_t grid_h, uint32_t* map);
// one step of the pull rule over queue[0, n): sets flags in `active`, never clears one
void pull(hipStream_t stream, const uint2* queue, uint32_t n, const uint32_t* map, uint32_t grid_w, uint32_t grid_h, const uint32_t* samples,
          uint32_t* active, uint32_t max_ratio, uint32_t max_spp);
// the flagged tiles of queue[0, n) with samples == n_level, in queue order, into out_tiles / out_q, their number into *count
void compact_level(hipStream_t stream, const uint2* queue, const uint32_t* active, const uint32_t* samples, uint32_t n_level, uint32_t n,
                   uint2* out_tiles, uint32_t* out_q, uint32_t* count);
}  // namespace tr_nbound
