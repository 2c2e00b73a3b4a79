// Host emulation of the kernels of the filtered stopping rule (tray_rust_amd/csrc/hip/guide_kernels.h): k_dn_filter_halves, k_guide_mark and
// k_guide_compact, compiled by g++ behind hip_emu.h and run as SIMT fibers, so that the LDS staging, the barriers, the ballots and the
// block-wide scan execute as the device executes them. Built by tests/test_guide_emu.py.
#include "hip_emu.h"
#include "../../tray_rust_amd/csrc/hip/guide_kernels.h"

#include <vector>

using namespace tr_denoise;
using namespace tr_guide;

template <int F>
static int filter_halves(const float4* scratch, uint32_t width, uint32_t height, uint32_t radius, float k, const uint32_t* blocks, uint32_t grid, float4* fa,
                         float4* fb) {
    return hip_emu::launch_simt(grid, DN_BLOCK, [&] { k_dn_filter_halves<F>(scratch, width, height, radius, k, blocks, fa, fb); });
}

extern "C" {

// the launches of one tray_denoise_halves_device call, in its order (k_dn_prepare<0>, <1>, k_dn_filter_halves<patch> over the list, or over every
// block when blocks is null); scratch: 48 bytes per pixel
int emu_guide_halves(const float* even, const float* odd, uint32_t width, uint32_t height, uint32_t radius, uint32_t patch, float k, const uint32_t* blocks,
                     uint32_t n_blocks, float* fa, float* fb, void* scratch) {
    if (width == 0u || height == 0u || radius < 1u || radius > DN_RMAX || patch > DN_FMAX) return -2;
    if (blocks && n_blocks == 0u) return 0;
    const float4* const e4 = reinterpret_cast<const float4*>(even);
    const float4* const o4 = reinterpret_cast<const float4*>(odd);
    float4* const s4 = static_cast<float4*>(scratch);
    float4* const a4 = reinterpret_cast<float4*>(fa);
    float4* const b4 = reinterpret_cast<float4*>(fb);
    const uint32_t prep = (uint32_t)(((uint64_t)width * height + DN_PREP_BLOCK - 1u) / DN_PREP_BLOCK);
    int rc = hip_emu::launch_simt(prep, DN_PREP_BLOCK, [&] { k_dn_prepare<0>(e4, o4, width, height, s4); });
    if (rc == 0) rc = hip_emu::launch_simt(prep, DN_PREP_BLOCK, [&] { k_dn_prepare<1>(e4, o4, width, height, s4); });
    if (rc != 0) return rc;
    const uint32_t grid = blocks ? n_blocks : dn_tiles_x(width) * dn_tiles_y(height);
    switch (patch) {
        case 0u: return filter_halves<0>(s4, width, height, radius, k, blocks, grid, a4, b4);
        case 1u: return filter_halves<1>(s4, width, height, radius, k, blocks, grid, a4, b4);
        case 2u: return filter_halves<2>(s4, width, height, radius, k, blocks, grid, a4, b4);
        default: return filter_halves<3>(s4, width, height, radius, k, blocks, grid, a4, b4);
    }
}

// one k_guide_mark launch as guide.hip makes it; queue_xy: n (x, y) pairs, active: n words or null; flags: one word per block of the frame
int emu_guide_mark(const uint32_t* queue_xy, const uint32_t* active, uint32_t n, uint32_t width, uint32_t height, uint32_t* flags) {
    if (n == 0u) return 0;   // (the library never launches over an empty queue)
    std::vector<uint2> queue(n);
    for (uint32_t i = 0; i < n; ++i) queue[i] = make_uint2(queue_xy[2 * i], queue_xy[2 * i + 1]);
    return hip_emu::launch_simt((n + GD_MARK_BLOCK - 1u) / GD_MARK_BLOCK, GD_MARK_BLOCK,
                                [&] { k_guide_mark(queue.data(), active, n, dn_tiles_x(width), dn_tiles_y(height), flags); });
}

// one k_guide_compact launch as guide.hip makes it
int emu_guide_compact(const uint32_t* flags, uint32_t width, uint32_t height, uint32_t* list, uint32_t* count) {
    return hip_emu::launch_simt(1u, GD_COMPACT_BLOCK, [&] { k_guide_compact(flags, dn_tiles_x(width) * dn_tiles_y(height), list, count); });
}

}  // extern "C"
