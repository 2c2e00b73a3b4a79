// libtrayhip_ranges.so: the sample-range instantiations of the tile kernel, the wavefront schedule's round head and the sampler pass
// (kernel_ranges.h), in groups that compile side by side:
//   hipcc -DTR_RANGE_GROUP=<0 | 1 | 2> -c kernel_ranges.hip -o kranges_<g>.o
// Group 0: k_path_tiles of static scenes, 1: of moving scenes, 2: k_wf_advance and k_sampler_pass.
#ifndef TR_RANGE_GROUP
#error "compile with -DTR_RANGE_GROUP=<0 .. 2> (csrc/Makefile)"
#endif
#define TR_DEVICE_TU
#define TR_SAMPLE_RANGES
#include "kernels.hip"
#include "kernel_ranges.h"

namespace tr_ranges {

#if TR_RANGE_GROUP == 0 || TR_RANGE_GROUP == 1
#define RANGE_TILES_L(A, F, L) hipLaunchKernelGGL((k_path_tiles<A, F, TRAY_INTEGRATOR_PATH, L>), grid, block, lds, stream, dev, tiles, tile_count, chunk, chunk_stride, \
                                                  spp, kf, levels, rgbw, counter, stats, smp_begin, smp_end)
#define RANGE_TILES(A, F) do { if (light_filter) RANGE_TILES_L(A, F, true); else RANGE_TILES_L(A, F, false); } while (0)
#define RANGE_TILES_F(A) do { if (whitted) hipLaunchKernelGGL((k_path_tiles<A, FEAT_ALL | FEAT_TEX, TRAY_INTEGRATOR_WHITTED>), grid, block, lds, stream, dev, tiles, \
                                                              tile_count, chunk, chunk_stride, spp, kf, levels, rgbw, counter, stats, smp_begin, smp_end); \
                              else if (feat == FEAT_NONE) RANGE_TILES(A, FEAT_NONE); else if (feat == FEAT_MERL) RANGE_TILES(A, FEAT_MERL); \
                              else if (feat == FEAT_SPEC) RANGE_TILES(A, FEAT_SPEC); else if (feat == (FEAT_MERL | FEAT_SPEC)) RANGE_TILES(A, FEAT_MERL | FEAT_SPEC); \
                              else if (feat == (FEAT_ALL | FEAT_TEX)) RANGE_TILES(A, FEAT_ALL | FEAT_TEX); else RANGE_TILES(A, FEAT_ALL); } while (0)
// (group 0 defines path_tiles and launches the static instantiations; the moving ones are group 1's, reached through path_tiles_moving)
#if TR_RANGE_GROUP == 1
void path_tiles_moving(int feat, bool whitted, bool light_filter, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const tr::DevScene& dev,
                       const uint2* tiles, uint32_t tile_count, uint32_t chunk, uint32_t chunk_stride, uint32_t spp, uint32_t kf, uint32_t levels, float* rgbw,
                       uint32_t* counter, DevStats* stats, uint32_t smp_begin, uint32_t smp_end) {
    RANGE_TILES_F(1);
}
#else
void path_tiles_moving(int feat, bool whitted, bool light_filter, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const tr::DevScene& dev,
                       const uint2* tiles, uint32_t tile_count, uint32_t chunk, uint32_t chunk_stride, uint32_t spp, uint32_t kf, uint32_t levels, float* rgbw,
                       uint32_t* counter, DevStats* stats, uint32_t smp_begin, uint32_t smp_end);
void path_tiles(int anim, int feat, bool whitted, bool light_filter, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const tr::DevScene& dev,
                const uint2* tiles, uint32_t tile_count, uint32_t chunk, uint32_t chunk_stride, uint32_t spp, uint32_t kf, uint32_t levels, float* rgbw,
                uint32_t* counter, DevStats* stats, uint32_t smp_begin, uint32_t smp_end) {
    if (anim) { path_tiles_moving(feat, whitted, light_filter, grid, block, lds, stream, dev, tiles, tile_count, chunk, chunk_stride, spp, kf, levels, rgbw, counter, stats, smp_begin, smp_end); return; }
    RANGE_TILES_F(0);
}
#endif
#undef RANGE_TILES_F
#undef RANGE_TILES
#undef RANGE_TILES_L
#endif

#if TR_RANGE_GROUP == 2
void wf_advance(int anim, dim3 grid, dim3 block, hipStream_t stream, const tr::DevScene& dev, const tr::WfPool& pool, tr::WfChunk* chunks, float* bins,
                const uint2* tiles, uint32_t tile_count, uint32_t chunk, uint32_t chunk_stride, uint32_t spp, uint32_t kf, float* rgbw,
                uint32_t* tile_counter, uint32_t* tiles_done, DevStats* stats, uint32_t* queue_a, uint32_t* queue_r, uint32_t* qctl,
                uint32_t slice_shift, uint32_t smp_begin, uint32_t smp_end) {
    if (anim) hipLaunchKernelGGL(tr::k_wf_advance<1>, grid, block, 0, stream, dev, pool, chunks, bins, tiles, tile_count, chunk, chunk_stride, spp, kf, rgbw,
                                 tile_counter, tiles_done, stats, queue_a, queue_r, qctl, slice_shift, smp_begin, smp_end);
    else hipLaunchKernelGGL(tr::k_wf_advance<0>, grid, block, 0, stream, dev, pool, chunks, bins, tiles, tile_count, chunk, chunk_stride, spp, kf, rgbw,
                            tile_counter, tiles_done, stats, queue_a, queue_r, qctl, slice_shift, smp_begin, smp_end);
}

void sampler_pass(int anim, bool lean, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const tr::DevScene& dev, const uint2* tiles,
                  uint32_t item0, uint32_t n_items, uint32_t chunk, uint32_t chunk_stride, uint32_t kf, const SamplerPass& sp,
                  const uint32_t* px_state, float* px_lum, float* rgbw, DevStats* stats, uint32_t group, uint32_t smp_first) {
#define RANGE_PASS(A, F) hipLaunchKernelGGL((k_sampler_pass<A, F>), grid, block, lds, stream, dev, tiles, item0, n_items, chunk, chunk_stride, kf, sp, px_state, \
                                            px_lum, rgbw, stats, group, smp_first)
    if (anim == 3) { if (lean) RANGE_PASS(3, FEAT_NONE); else RANGE_PASS(3, FEAT_ALL | FEAT_TEX); }
    else if (anim == 2) { if (lean) RANGE_PASS(2, FEAT_NONE); else RANGE_PASS(2, FEAT_ALL | FEAT_TEX); }
    else { if (lean) RANGE_PASS(0, FEAT_NONE); else RANGE_PASS(0, FEAT_ALL | FEAT_TEX); }
#undef RANGE_PASS
}
#endif

}  // namespace tr_ranges
