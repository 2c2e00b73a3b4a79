// The lean tile kernel (libtrayhip_tiles.so): the instantiations k_path_tiles<0, FEAT, TRAY_INTEGRATOR_PATH, LFILT> of static scenes, compiled from
// kernel_tiles.hip with TR_LEAN_TILES defined; device_api.hip launches them through these functions. libtrayhip.so's own code objects stay the base
// kernel's, which is the fallback (TRAYHIP_LEAN_TILES=0) and what moving scenes, Whitted and the sample-range launches run.
//
// TR_LEAN_TILES is where tile-kernel performance work goes: every edit to kernels.hip and the dev_*.h headers sits inside a sub-macro that
// TR_LEAN_TILES turns on (dev_integrator.h lists them), with the existing text as the #else, so the base stays what its recorded hash stands for.
// The rule of every item: each camera sample's radiance and the launch's sample, vertex and ray counts keep their bits (tests/test_lean_tiles_emu.py).
// A re-timed item (TR_LEAN_FOLD_MIS_RAY) keeps them too and moves only the step a sample finishes in, i.e. the order of the film's f32 sums
// (tests/test_lean_fold_emu.py, tests/test_gpu_lean_fold.py). It is not compiled into this library, whose code objects stay what their recorded hash
// stands for: the instantiations it applies to -- LFILT = false -- are compiled with it into libtrayhip_foldmis.so (kernel_fold.h), and path_tiles /
// path_tiles_kernel hand the launches without mis_ray_filter on to that library.
#pragma once

namespace tr_tiles {
void path_tiles(int feat, bool light_filter, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const tr::DevScene& dev, const uint2* tiles,
                uint32_t tile_count, uint32_t chunk, uint32_t chunk_stride, uint32_t spp, uint32_t kf, uint32_t levels, float* rgbw, uint32_t* counter,
                DevStats* stats);
// the kernel path_tiles launches: what the occupancy is asked of
const void* path_tiles_kernel(int feat, bool light_filter);
// (their halves for the lobe sets beyond FEAT_NONE: the seam between the two translation units the library compiles as)
void path_tiles_lobes(int feat, bool light_filter, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const tr::DevScene& dev, const uint2* tiles,
                      uint32_t tile_count, uint32_t chunk, uint32_t chunk_stride, uint32_t spp, uint32_t kf, uint32_t levels, float* rgbw,
                      uint32_t* counter, DevStats* stats);
const void* path_tiles_kernel_lobes(int feat, bool light_filter);
}  // namespace tr_tiles
