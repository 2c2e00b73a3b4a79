// libtrayhip_tiles.so: the tile kernel's path-tracer instantiations of static scenes, compiled lean (kernel_tiles.h), in groups that compile
// side by side:
//   hipcc -DTR_TILES_GROUP=<0 | 1> -c kernel_tiles.hip -o ktiles_<g>.o
// Group 0: k_path_tiles<0, FEAT_NONE, PATH, LFILT> (with group 0's scheduling strategy: csrc/Makefile), 1: every other lobe set of kernel_list.h.
#ifndef TR_TILES_GROUP
#error "compile with -DTR_TILES_GROUP=<0 | 1> (csrc/Makefile)"
#endif
#define TR_DEVICE_TU
#define TR_LEAN_TILES
#include "kernels.hip"
#include "kernel_select.h"
#include "kernel_tiles.h"
#include "kernel_fold.h"

namespace tr_tiles {

#if TR_TILES_GROUP == 0
// (group 0 defines the entry points; the lobe sets beyond FEAT_NONE are group 1's)
// TRAYHIP_LEAN_FOLD=0: the launches without mis_ray_filter stay in this library (read at every call, like TRAYHIP_LEAN_TILES before the device scene is created:
// path_tiles_kernel names the kernel whose launch attributes are set then)
static bool folds() { const char* e = getenv("TRAYHIP_LEAN_FOLD"); return !e || atoi(e) != 0; }
void path_tiles(int feat, bool light_filter, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const tr::DevScene& dev, const uint2* tiles,
                uint32_t tile_count, uint32_t chunk, uint32_t chunk_stride, uint32_t spp, uint32_t kf, uint32_t levels, float* rgbw, uint32_t* counter,
                DevStats* stats) {
    // the instantiations without mis_ray_filter run from libtrayhip_foldmis.so, which compiles them with the re-timed item as well (kernel_fold.h);
    // this library's own copies of them -- every item but the re-timed one -- are what TRAYHIP_LEAN_FOLD=0 runs (A/B runs, bisecting)
    if (!light_filter && folds()) {
        if (getenv("TRAYHIP_STATS")) fprintf(stderr, "[trayhip] lean tile kernel: the folding instantiation (libtrayhip_foldmis.so)\n");
        tr_fold::path_tiles(feat, grid, block, lds, stream, dev, tiles, tile_count, chunk, chunk_stride, spp, kf, levels, rgbw, counter, stats);
        return;
    }
    if (feat != FEAT_NONE) { path_tiles_lobes(feat, light_filter, grid, block, lds, stream, dev, tiles, tile_count, chunk, chunk_stride, spp, kf, levels, rgbw, counter, stats); return; }
    select_path_tiles_filter<0, FEAT_NONE>(light_filter, [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, dev, tiles, tile_count, chunk, chunk_stride, spp, kf, levels, rgbw, counter, stats);
    });
}
const void* path_tiles_kernel(int feat, bool light_filter) {
    if (!light_filter && folds()) return tr_fold::path_tiles_kernel(feat);
    if (feat != FEAT_NONE) return path_tiles_kernel_lobes(feat, light_filter);
    const void* k = nullptr;
    select_path_tiles_filter<0, FEAT_NONE>(light_filter, [&](auto kernel) { k = reinterpret_cast<const void*>(kernel); });
    return k;
}
#else
// select_path_tiles' lobe sets (kernel_select.h) without FEAT_NONE and Whitted
template <class F>
static void select_lobes(int feat, bool light_filter, F&& f) {
    if (feat == FEAT_MERL) select_path_tiles_filter<0, FEAT_MERL>(light_filter, f);
    else if (feat == FEAT_SPEC) select_path_tiles_filter<0, FEAT_SPEC>(light_filter, f);
    else if (feat == (FEAT_MERL | FEAT_SPEC)) select_path_tiles_filter<0, FEAT_MERL | FEAT_SPEC>(light_filter, f);
    else if (feat == (FEAT_ALL | FEAT_TEX)) select_path_tiles_filter<0, FEAT_ALL | FEAT_TEX>(light_filter, f);
    else select_path_tiles_filter<0, FEAT_ALL>(light_filter, f);
}
void path_tiles_lobes(int feat, bool light_filter, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const tr::DevScene& dev, const uint2* tiles,
                      uint32_t tile_count, uint32_t chunk, uint32_t chunk_stride, uint32_t spp, uint32_t kf, uint32_t levels, float* rgbw,
                      uint32_t* counter, DevStats* stats) {
    select_lobes(feat, light_filter, [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, dev, tiles, tile_count, chunk, chunk_stride, spp, kf, levels, rgbw, counter, stats);
    });
}
const void* path_tiles_kernel_lobes(int feat, bool light_filter) {
    const void* k = nullptr;
    select_lobes(feat, light_filter, [&](auto kernel) { k = reinterpret_cast<const void*>(kernel); });
    return k;
}
#endif

}  // namespace tr_tiles
