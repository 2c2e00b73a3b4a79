// Host emulation of the first-hit kernels (tray_rust_amd/csrc/hip/first_hit_kernels.h): k_debug_first_hit one thread at a time, k_first_hit_tiles as
// SIMT fibers (256 per workgroup: the wave-uniform sample loop, the LDS window, the barrier and the flush run as the device runs them), and the
// two element-wise kernels of tray_denoise_demodulated_device. Built by tests/_first_hit_ref.py over emu_kernels.cpp, whose scene set-up it uses;
// the launches follow device_api.hip's: the ANIM set of the debug kernels and the scene's own dynamic LDS, both from its plan (scene_plan.h).
#include "emu_kernels.cpp"
#include "../../tray_rust_amd/csrc/hip/first_hit_kernels.h"

extern "C" {

// k_debug_first_hit for n (pixel, sample) items (what tray_debug_first_hit launches): twelve floats per item
int emu_debug_first_hit(const TrayFlatScene* f, uint32_t n, const uint32_t* px, const uint32_t* py, const uint32_t* si, uint32_t spp, uint64_t seed,
                        float* out) {
    EmuScene e;
    make_scene(f, e);
    const uint32_t kf = tr_rules::frame_key(seed, e.d.frame);
    const uint32_t grid = (n + TR_BLOCK - 1) / TR_BLOCK;
    const int anim = e.plan.anim_debug();
    if (anim == 3) launch(grid, TR_BLOCK, [&] { k_debug_first_hit<3>(e.d, n, px, py, si, spp, kf, out); });
    else if (anim) launch(grid, TR_BLOCK, [&] { k_debug_first_hit<2>(e.d, n, px, py, si, spp, kf, out); });
    else launch(grid, TR_BLOCK, [&] { k_debug_first_hit<0>(e.d, n, px, py, si, spp, kf, out); });
    return 0;
}

// one k_first_hit_tiles launch over the given tiles (what tray_render_first_hit_device launches); the three films are accumulated into.
// Returns 0, or -3 if a rendezvous could not complete.
int emu_render_first_hit(const TrayFlatScene* f, const uint32_t* tiles_xy, uint32_t tile_count, uint32_t spp, uint32_t smp_begin, uint32_t smp_end,
                         uint64_t seed, float* albedo, float* normal, float* depth) {
    if (tile_count == 0u) return 0;
    EmuScene e;
    make_scene(f, e);
    lds_layout(f, e, true, true);
    std::vector<uint2> tiles(tile_count);
    for (uint32_t i = 0; i < tile_count; ++i) tiles[i] = make_uint2(tiles_xy[2 * i], tiles_xy[2 * i + 1]);
    const uint32_t kf = tr_rules::frame_key(seed, e.d.frame);
    const int anim = e.plan.anim_debug();
    const size_t lds = e.plan.stack_bytes;
    if (anim == 3) return launch_simt(tile_count, TR_BLOCK, [&] { k_first_hit_tiles<3>(e.d, tiles.data(), spp, kf, smp_begin, smp_end, albedo, normal, depth); }, lds);
    if (anim) return launch_simt(tile_count, TR_BLOCK, [&] { k_first_hit_tiles<2>(e.d, tiles.data(), spp, kf, smp_begin, smp_end, albedo, normal, depth); }, lds);
    return launch_simt(tile_count, TR_BLOCK, [&] { k_first_hit_tiles<0>(e.d, tiles.data(), spp, kf, smp_begin, smp_end, albedo, normal, depth); }, lds);
}

// k_fh_demodulate / k_fh_remodulate over n_px pixels, as first_hit.hip launches them
int emu_fh_demodulate(const float* even, const float* odd, const float* albedo, uint32_t n_px, float* even_out, float* odd_out) {
    launch((n_px + TR_BLOCK - 1) / TR_BLOCK, TR_BLOCK, [&] {
        k_fh_demodulate(reinterpret_cast<const float4*>(even), reinterpret_cast<const float4*>(odd), reinterpret_cast<const float4*>(albedo), n_px,
                        reinterpret_cast<float4*>(even_out), reinterpret_cast<float4*>(odd_out));
    });
    return 0;
}
int emu_fh_remodulate(const float* albedo, uint32_t n_px, float* out) {
    launch((n_px + TR_BLOCK - 1) / TR_BLOCK, TR_BLOCK, [&] { k_fh_remodulate(reinterpret_cast<const float4*>(albedo), n_px, reinterpret_cast<float4*>(out)); });
    return 0;
}

}  // extern "C"
