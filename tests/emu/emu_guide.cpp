// Host emulation of the kernels of the filtered stopping rule (tray_rust_amd/csrc/hip/guide_kernels.h): k_dn_filter_halves, k_guide_mark and
// k_guide_compact, compiled by g++ behind hip_emu.h and run as SIMT fibers, so that the LDS staging, the barriers, the ballots and the
// block-wide scan execute as the device executes them. Built by tests/test_guide_emu.py. Includes emu_denoise.cpp for EmuOps.
#include "emu_denoise.cpp"
#include "../../tray_rust_amd/csrc/hip/guide_kernels.h"

#include <vector>

using namespace tr_guide;

struct GuideOps : EmuOps {
    using EmuOps::EmuOps;
    // one k_dn_filter_halves<patch> launch as guide.hip makes it: over the list, or over every block when blocks is null
    void halves(const void* records, uint32_t radius, uint32_t patch, float k, const uint32_t* blocks, uint32_t n_blocks, float* fa, float* fb) {
        const float4* const s4 = emu_f4(records);
        float4* const a4 = emu_f4(fa), * const b4 = emu_f4(fb);
        run_tiles(blocks ? n_blocks : dn_tiles_x(width) * dn_tiles_y(height), patch,
                  [&](auto f) { k_dn_filter_halves<decltype(f)::value>(s4, width, height, radius, k, blocks, a4, b4); });
    }
};

extern "C" {

// one tray_denoise_halves_device call: the plan's schedule (k_dn_prepare<0>, <1>, k_dn_filter_halves<patch>; nothing for an empty list); scratch: 48
// bytes per pixel
int emu_guide_halves(const float* even, const float* odd, uint32_t width, uint32_t height, uint32_t radius, uint32_t patch, float k, const uint32_t* blocks,
                     uint32_t n_blocks, float* fa, float* fb, void* scratch) {
    const dn::Params p{radius, 0u, patch, k};
    if (emu_refused(emu_filter_args(width, height, p))) return -2;
    GuideOps ops(width, height);
    dn::halves(ops, dn::Frame{even, odd, nullptr, nullptr, nullptr}, p, blocks, n_blocks, fa, fb, scratch);
    return ops.rc;
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
