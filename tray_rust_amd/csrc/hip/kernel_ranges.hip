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
#include "kernel_select.h"

namespace tr_ranges {

// (group 0 defines path_tiles and launches the static instantiations; the moving ones are group 1's, reached through path_tiles_moving)
#if TR_RANGE_GROUP == 1
void path_tiles_moving(int feat, bool whitted, bool light_filter, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const tr::DevScene& dev,
                       const uint2* tiles, uint32_t tile_count, uint32_t chunk, uint32_t chunk_stride, uint32_t spp, uint32_t kf, uint32_t levels, float* rgbw,
                       uint32_t* counter, DevStats* stats, uint32_t smp_begin, uint32_t smp_end) {
    select_path_tiles<1>(feat, whitted, light_filter, [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, dev, tiles, tile_count, chunk, chunk_stride, spp, kf, levels, rgbw, counter, stats, smp_begin, smp_end);
    });
}
#elif TR_RANGE_GROUP == 0
void path_tiles(int anim, int feat, bool whitted, bool light_filter, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const tr::DevScene& dev,
                const uint2* tiles, uint32_t tile_count, uint32_t chunk, uint32_t chunk_stride, uint32_t spp, uint32_t kf, uint32_t levels, float* rgbw,
                uint32_t* counter, DevStats* stats, uint32_t smp_begin, uint32_t smp_end) {
    if (anim) { path_tiles_moving(feat, whitted, light_filter, grid, block, lds, stream, dev, tiles, tile_count, chunk, chunk_stride, spp, kf, levels, rgbw, counter, stats, smp_begin, smp_end); return; }
    select_path_tiles<0>(feat, whitted, light_filter, [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, dev, tiles, tile_count, chunk, chunk_stride, spp, kf, levels, rgbw, counter, stats, smp_begin, smp_end);
    });
}
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
    select_sampler_pass(anim, lean, [&](auto kernel) {
        hipLaunchKernelGGL(kernel, grid, block, lds, stream, dev, tiles, item0, n_items, chunk, chunk_stride, kf, sp, px_state, px_lum, rgbw, stats, group, smp_first);
    });
}
#endif

}  // namespace tr_ranges
