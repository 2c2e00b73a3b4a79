// Host emulation of the kernels of tray_denoise_guided_device and tray_denoise_two_pass_device (tray_rust_amd/csrc/hip/guided_kernels.h):
// k_dn_prepare, k_dn_filter_halves and k_gdn_filter, compiled by g++ behind hip_emu.h and run as SIMT fibers, so that the LDS staging of the guide,
// the two barriers per offset, the separable patch sums and the values' loads execute as the device executes them. Built by
// tests/_guided_ref.py. Includes emu_guide.cpp for GuideOps (EmuOps and k_dn_filter_halves).
#include "emu_guide.cpp"
#include "../../tray_rust_amd/csrc/hip/guided_kernels.h"

using namespace tr_guided;

struct GuidedOps : GuideOps {
    using GuideOps::GuideOps;
    // one k_gdn_filter<patch> launch as guided.hip makes it
    void filter(const void* guide, const void* values, uint32_t radius, uint32_t patch, float k, float* out) {
        const float4* const g4 = emu_f4(guide), * const v4 = emu_f4(values);
        float4* const out4 = emu_f4(out);
        run_tiles(patch, [&](auto f) { k_gdn_filter<decltype(f)::value>(g4, v4, width, height, radius, k, out4); });
    }
};

extern "C" {

uint64_t emu_guided_scratch_bytes(uint32_t width, uint32_t height) { return gdn_scratch_bytes(width, height); }
uint64_t emu_two_pass_scratch_bytes(uint32_t width, uint32_t height) { return gdn_two_pass_scratch_bytes(width, height); }

// one tray_denoise_guided_device call: the plan's schedule (five launches) and scratch layout
int emu_denoise_guided(uint32_t width, uint32_t height, const float* even, const float* odd, const float* guide_a, const float* guide_b, uint32_t radius,
                       uint32_t patch, float k, float* out, void* scratch) {
    const dn::Params p{radius, 0u, patch, k};
    if (emu_refused(emu_filter_args(width, height, p))) return -2;
    GuidedOps ops(width, height);
    dn::guided(ops, dn::Frame{even, odd, nullptr, guide_a, guide_b}, p, out, scratch);
    return ops.rc;
}

// one tray_denoise_two_pass_device call: the plan's schedule (six launches) and scratch layout
int emu_denoise_two_pass(uint32_t width, uint32_t height, const float* even, const float* odd, uint32_t radius, uint32_t patch, float k, uint32_t radius2,
                         uint32_t patch2, float k2, float* out, void* scratch) {
    const dn::Params p{radius, 0u, patch, k}, second{radius2, 0u, patch2, k2};
    if (emu_refused(emu_filter_args(width, height, p)) || emu_refused(emu_filter_args(width, height, second))) return -2;
    GuidedOps ops(width, height);
    dn::two_pass(ops, dn::Frame{even, odd, nullptr, nullptr, nullptr}, p, second, out, scratch);
    return ops.rc;
}

}  // extern "C"
