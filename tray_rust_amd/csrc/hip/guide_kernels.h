// The kernels that let tray_render_noise_target_filtered_device stop on the error of the denoised image (include/trayhip.h): k_dn_filter_halves
// writes the two cross-filtered halves of the dual-buffer filter as films of their own, over the whole frame or over a list of 32 x 16 blocks;
// k_guide_mark and k_guide_compact make the next round's list from the active tiles. Device code only; compiled into libtrayhip_guide.so by
// guide.hip, and by g++ into the host emulation (tests/emu/emu_guide.cpp).
//
// k_dn_filter_halves is k_dn_filter (denoise_kernels.h) with another front and another end around the one body, dn_filter_block: the block
// index comes from a list (or is blockIdx.x), and where k_dn_filter stores ((A + B) / 2, 1) this one stores fa = (A, wA) and fb = (B, wB), two
// float4 stores per thread. (fa.rgb + fb.rgb) * 0.5f is therefore k_dn_filter's out.rgb to the bit; tests/test_guide_emu.py and
// tests/test_gpu_guide.py compare the two.
// Barriers: an index outside the frame's blocks ends the whole workgroup before the call of dn_filter_block, that is, before the first
// barrier; every other workgroup calls it with all its threads, whatever the list holds. Stores are bounded by the image.
#pragma once
#include "block_compact.h"
#include "denoise_kernels.h"

namespace tr_guide {

using namespace tr_denoise;

#define GD_MARK_BLOCK 256u      // k_guide_mark: one thread per queue entry
#define GD_COMPACT_BLOCK 1024u  // k_guide_compact: the one workgroup

template <int F>
__global__ __launch_bounds__(DN_BLOCK) void k_dn_filter_halves(const float4* __restrict__ scratch, uint32_t width, uint32_t height, uint32_t radius,
                                                               float k, const uint32_t* __restrict__ blocks, float4* __restrict__ fa,
                                                               float4* __restrict__ fb) {
    const uint32_t block = blocks ? blocks[blockIdx.x] : blockIdx.x;
    if (block >= dn_tiles_x(width) * dn_tiles_y(height)) return;   // (the same for every thread of the workgroup)
    const dn_halves h = dn_normalise(dn_filter_block<F>(scratch, nullptr, nullptr, width, height, radius, k, block, nullptr));
    if (h.px < width && h.py < height) {
        fa[(size_t)h.py * width + h.px] = h.A;
        fb[(size_t)h.py * width + h.px] = h.B;
    }
}

// The 32 x 16 blocks that hold a tile of queue[0, n) whose flag is set (active == null: every tile of the queue): flags[block] = 1, the block
// row-major over blocks_x blocks per row. A block holds 4 x 2 tiles of 8 x 8 pixels. Several threads may store the same word; all store 1.
// Tiles whose block lies outside the blocks_x x blocks_y grid are passed over.
__global__ __launch_bounds__(GD_MARK_BLOCK) void k_guide_mark(const uint2* __restrict__ queue, const uint32_t* __restrict__ active, uint32_t n,
                                                              uint32_t blocks_x, uint32_t blocks_y, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * GD_MARK_BLOCK + threadIdx.x;
    if (i >= n || (active && active[i] == 0u)) return;
    const uint2 tile = queue[i];
    const uint32_t bx = tile.x / (DN_TW / 8u), by = tile.y / (DN_TH / 8u);
    if (bx < blocks_x && by < blocks_y) flags[by * blocks_x + bx] = 1u;
}

// The indices of the set flags of flags[0, n) in rising order into list, their number into *count: one workgroup walks the flags in steps of
// GD_COMPACT_BLOCK (block_compact.h; the loop's bound is uniform).
__global__ __launch_bounds__(GD_COMPACT_BLOCK) void k_guide_compact(const uint32_t* __restrict__ flags, uint32_t n, uint32_t* __restrict__ list,
                                                                    uint32_t* __restrict__ count) {
    __shared__ uint32_t s_wave[GD_COMPACT_BLOCK / 64u];
    uint32_t total = 0u;
    for (uint32_t i0 = 0u; i0 < n; i0 += GD_COMPACT_BLOCK) {
        const uint32_t i = i0 + threadIdx.x;
        const bool keep = i < n && flags[i] != 0u;
        const uint32_t o = tr::block_compact_slot<GD_COMPACT_BLOCK>(keep, total, s_wave);
        if (keep) list[o] = i;   // (o < n: at most one entry per flag)
    }
    if (threadIdx.x == 0u) *count = total;
}

}  // namespace tr_guide
