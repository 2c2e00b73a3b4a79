// libtrayhip_foldmis.so: the lean tile kernel's instantiations WITHOUT mis_ray_filter, k_path_tiles<0, FEAT, TRAY_INTEGRATOR_PATH, false>, compiled from
// kernel_fold.hip with TR_LEAN_TILES and its re-timed item TR_LEAN_FOLD_MIS_RAY (dev_integrator.h) defined. libtrayhip_tiles.so's entry points
// (kernel_tiles.hip) hand the launches with light_filter == false on to these functions; its own code objects -- every item but the re-timed one, in
// all instantiations -- stay what its recorded hash stands for, and its LFILT kernels are what scenes with a sphere light or specular lobes run.
#pragma once

namespace tr_fold {
void path_tiles(int feat, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const tr::DevScene& dev, const uint2* tiles, uint32_t tile_count,
                uint32_t chunk, uint32_t chunk_stride, uint32_t spp, uint32_t kf, uint32_t levels, float* rgbw, uint32_t* counter, DevStats* stats);
// the kernel path_tiles launches: what the occupancy is asked of
const void* path_tiles_kernel(int feat);
// (their halves for the lobe sets beyond FEAT_NONE: the seam between the two translation units the library compiles as)
void path_tiles_lobes(int feat, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const tr::DevScene& dev, const uint2* tiles, uint32_t tile_count,
                      uint32_t chunk, uint32_t chunk_stride, uint32_t spp, uint32_t kf, uint32_t levels, float* rgbw, uint32_t* counter, DevStats* stats);
const void* path_tiles_kernel_lobes(int feat);
}  // namespace tr_fold
