// Host emulation of the sample-range launches (tray_render_samples_device): the entry points of emu_kernels.cpp for the tile kernel, the
// wavefront schedule and the sampler pass, with the range [smp_begin, smp_end) of the spp-sample LowDiscrepancy frame handed to the kernels
// as device_api.hip hands it (0 / 0, or [0, spp): the whole frame) and the launch rules (levels, slice_shift, rounds) applied to its n samples.
// Built by tests/test_sample_ranges_emu.py: the same device sources as libtrayemu.so, with the range arguments of libtrayhip_ranges.so's
// instantiations (TR_SAMPLE_RANGES; emu_kernels.cpp's own entry points pass none and render whole frames).
#define TR_SAMPLE_RANGES
#include "emu_kernels.cpp"

extern "C" {

// emu_render_tiles over a sample range (no shards)
int emu_render_tiles_range(const TrayFlatScene* f, const uint32_t* tiles_xy, uint32_t tile_count, uint32_t spp, uint32_t smp_begin, uint32_t smp_end,
                           uint64_t seed, float* rgbw, uint32_t blocks, int coop, int film_rows, unsigned long long* stats_out) {
    return render_tiles(f, tiles_xy, tile_count, spp, smp_begin, smp_end, seed, rgbw, blocks, coop, film_rows, stats_out, 0u, 0u, 1u);
}

// emu_render_wavefront over a sample range (k_wf_trace_dyn, the whole stack in LDS)
int emu_render_wavefront_range(const TrayFlatScene* f, const uint32_t* tiles_xy, uint32_t tile_count, uint32_t spp, uint32_t smp_begin, uint32_t smp_end,
                               uint64_t seed, float* rgbw, uint32_t n_chunks, uint32_t trace_blocks, unsigned long long* stats_out) {
    return render_wavefront(f, tiles_xy, tile_count, spp, smp_begin, smp_end, seed, rgbw, 0, n_chunks, trace_blocks, 0u, stats_out);
}

// emu_render_sampler with the LowDiscrepancy sampler (scenes with an AnimatedMesh) over a sample range
int emu_render_sampler_range(const TrayFlatScene* f, const uint32_t* tiles_xy, uint32_t tile_count, uint32_t spp, uint32_t smp_begin, uint32_t smp_end,
                             uint64_t seed, float* rgbw, uint32_t batch_tiles, unsigned long long* stats_out) {
    return render_sampler(f, tiles_xy, tile_count, TRAY_SAMPLER_LOW_DISCREPANCY, spp, spp, smp_begin, smp_end, seed, rgbw, batch_tiles, stats_out);
}

}  // extern "C"
