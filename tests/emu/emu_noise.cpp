// Host emulation of the per-round kernels of tray_render_noise_target_device (tray_rust_amd/csrc/hip/noise_kernels.h): k_noise_error and
// k_noise_compact, compiled by g++ behind hip_emu.h and run as SIMT fibers, so that the shuffles, ballots and the block-wide scan execute as
// the device executes them. Built by tests/test_noise_target_emu.py.
#include "hip_emu.h"
#include "../../tray_rust_amd/csrc/hip/noise_kernels.h"

#include <vector>

extern "C" {

// one k_noise_error launch as noise.hip makes it; tiles_xy: n_active (x, y) pairs, qidx: their queue indices or null (0 .. n_active - 1)
int emu_noise_error(const float* even, const float* odd, uint32_t width, uint32_t height, const uint32_t* tiles_xy, const uint32_t* qidx,
                    uint32_t n_active, uint32_t n_taken, uint32_t max_spp, float threshold, float* err, uint32_t* active, uint32_t* samples) {
    std::vector<uint2> tiles(n_active);
    for (uint32_t i = 0; i < n_active; ++i) tiles[i] = make_uint2(tiles_xy[2 * i], tiles_xy[2 * i + 1]);
    const uint32_t per_block = NT_ERR_BLOCK / 64u;
    return hip_emu::launch_simt((n_active + per_block - 1u) / per_block, NT_ERR_BLOCK, [&] {
        tr_noise::k_noise_error(reinterpret_cast<const float4*>(even), reinterpret_cast<const float4*>(odd), width, height, tiles.data(), qidx, n_active,
                                n_taken, max_spp, threshold, err, active, samples);
    });
}

// one k_noise_compact launch as noise.hip makes it: the flagged entries of queue_xy[0, n) into out_xy / out_q, their number into *count
int emu_noise_compact(const uint32_t* queue_xy, const uint32_t* active, uint32_t n, uint32_t* out_xy, uint32_t* out_q, uint32_t* count) {
    std::vector<uint2> queue(n), out(n);
    for (uint32_t i = 0; i < n; ++i) queue[i] = make_uint2(queue_xy[2 * i], queue_xy[2 * i + 1]);
    const int rc = hip_emu::launch_simt(1u, NT_COMPACT_BLOCK, [&] { tr_noise::k_noise_compact(queue.data(), active, n, out.data(), out_q, count); });
    for (uint32_t i = 0; i < n; ++i) { out_xy[2 * i] = out[i].x; out_xy[2 * i + 1] = out[i].y; }
    return rc;
}

}  // extern "C"
