// libtrayhip_foldmis.so: the lean tile kernel's instantiations without mis_ray_filter, compiled with the re-timed item TR_LEAN_FOLD_MIS_RAY
// (kernel_fold.h), in groups that compile side by side as kernel_tiles.hip's:
//   hipcc -DTR_FOLD_GROUP=<0 | 1> -c kernel_fold.hip -o kfold_<g>.o
// Group 0: k_path_tiles<0, FEAT_NONE, PATH, false> (with group 0's scheduling strategy: csrc/Makefile), 1: every other lobe set of kernel_list.h.
#ifndef TR_FOLD_GROUP
#error "compile with -DTR_FOLD_GROUP=<0 | 1> (csrc/Makefile)"
#endif
#define TR_DEVICE_TU
#define TR_LEAN_TILES
#if !defined(TR_LEAN_PICK) && !defined(TR_LEAN_FOLD_MIS_RAY)   // the re-timed item (dev_integrator.h), which TR_LEAN_TILES does not turn on by itself
#define TR_LEAN_FOLD_MIS_RAY
#endif
#include "kernels.hip"
#include "kernel_fold.h"

namespace tr_fold {

#if TR_FOLD_GROUP == 0
// (group 0 defines the entry points; the lobe sets beyond FEAT_NONE are group 1's)
void path_tiles(int feat, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const tr::DevScene& dev, const uint2* tiles, uint32_t tile_count,
                uint32_t chunk, uint32_t chunk_stride, uint32_t spp, uint32_t kf, uint32_t levels, float* rgbw, uint32_t* counter, DevStats* stats) {
    if (feat != FEAT_NONE) { path_tiles_lobes(feat, grid, block, lds, stream, dev, tiles, tile_count, chunk, chunk_stride, spp, kf, levels, rgbw, counter, stats); return; }
    hipLaunchKernelGGL((k_path_tiles<0, FEAT_NONE, TRAY_INTEGRATOR_PATH, false>), grid, block, lds, stream, dev, tiles, tile_count, chunk, chunk_stride, spp, kf, levels, rgbw,
                       counter, stats);
}
const void* path_tiles_kernel(int feat) {
    if (feat != FEAT_NONE) return path_tiles_kernel_lobes(feat);
    return reinterpret_cast<const void*>(k_path_tiles<0, FEAT_NONE, TRAY_INTEGRATOR_PATH, false>);
}
#else
// select_path_tiles' lobe sets (kernel_select.h) without FEAT_NONE and Whitted, light_filter == false
template <class F>
static void select_lobes(int feat, F&& f) {
    if (feat == FEAT_MERL) f(k_path_tiles<0, FEAT_MERL, TRAY_INTEGRATOR_PATH, false>);
    else if (feat == FEAT_SPEC) f(k_path_tiles<0, FEAT_SPEC, TRAY_INTEGRATOR_PATH, false>);
    else if (feat == (FEAT_MERL | FEAT_SPEC)) f(k_path_tiles<0, FEAT_MERL | FEAT_SPEC, TRAY_INTEGRATOR_PATH, false>);
    else if (feat == (FEAT_ALL | FEAT_TEX)) f(k_path_tiles<0, FEAT_ALL | FEAT_TEX, TRAY_INTEGRATOR_PATH, false>);
    else f(k_path_tiles<0, FEAT_ALL, TRAY_INTEGRATOR_PATH, false>);
}
void path_tiles_lobes(int feat, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const tr::DevScene& dev, const uint2* tiles, uint32_t tile_count,
                      uint32_t chunk, uint32_t chunk_stride, uint32_t spp, uint32_t kf, uint32_t levels, float* rgbw, uint32_t* counter, DevStats* stats) {
    select_lobes(feat, [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, dev, tiles, tile_count, chunk, chunk_stride, spp, kf, levels, rgbw, counter, stats);
    });
}
const void* path_tiles_kernel_lobes(int feat) {
    const void* k = nullptr;
    select_lobes(feat, [&](auto kernel) { k = reinterpret_cast<const void*>(kernel); });
    return k;
}
#endif

}  // namespace tr_fold
