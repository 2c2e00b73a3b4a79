// The sample-range launches (tray_render_samples_device): the instantiations of k_path_tiles, k_wf_advance and k_sampler_pass that take a range
// [smp_begin, smp_end) of the spp-sample LowDiscrepancy frame (TR_SAMPLE_RANGES in kernels.hip / wavefront.h) live in libtrayhip_ranges.so,
// compiled from kernel_ranges.hip; device_api.hip launches them through these functions. libtrayhip.so's own code objects stay those of the
// whole-frame kernels. Each function picks the instantiation with the selector device_api.hip picks the whole-frame one with (kernel_select.h).
#pragma once

namespace tr_ranges {
void path_tiles(int anim, int feat, bool whitted, bool light_filter, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const tr::DevScene& dev,
                const uint2* tiles, uint32_t tile_count, uint32_t chunk, uint32_t chunk_stride, uint32_t spp, uint32_t kf, uint32_t levels, float* rgbw,
                uint32_t* counter, DevStats* stats, uint32_t smp_begin, uint32_t smp_end);
// (path_tiles' ANIM = 1 half: the seam between the two translation units the tile kernel's range instantiations compile as)
void path_tiles_moving(int feat, bool whitted, bool light_filter, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const tr::DevScene& dev,
                       const uint2* tiles, uint32_t tile_count, uint32_t chunk, uint32_t chunk_stride, uint32_t spp, uint32_t kf, uint32_t levels, float* rgbw,
                       uint32_t* counter, DevStats* stats, uint32_t smp_begin, uint32_t smp_end);
void wf_advance(int anim, dim3 grid, dim3 block, hipStream_t stream, const tr::DevScene& dev, const tr::WfPool& pool, tr::WfChunk* chunks, float* bins,
                const uint2* tiles, uint32_t tile_count, uint32_t chunk, uint32_t chunk_stride, uint32_t spp, uint32_t kf, float* rgbw,
                uint32_t* tile_counter, uint32_t* tiles_done, DevStats* stats, uint32_t* queue_a, uint32_t* queue_r, uint32_t* qctl,
                uint32_t slice_shift, uint32_t smp_begin, uint32_t smp_end);
void sampler_pass(int anim, bool lean, dim3 grid, dim3 block, size_t lds, hipStream_t stream, const tr::DevScene& dev, const uint2* tiles,
                  uint32_t item0, uint32_t n_items, uint32_t chunk, uint32_t chunk_stride, uint32_t kf, const SamplerPass& sp,
                  const uint32_t* px_state, float* px_lum, float* rgbw, DevStats* stats, uint32_t group, uint32_t smp_first);
}  // namespace tr_ranges
