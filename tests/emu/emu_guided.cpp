// Host emulation of the kernels of tray_denoise_guided_device and tray_denoise_two_pass_device (tray_rust_amd/csrc/hip/guided_kernels.h):
// k_dn_prepare, k_dn_filter_halves and k_gdn_filter, compiled by g++ behind hip_emu.h and run as SIMT fibers, so that the LDS staging of the guide,
// the two barriers per offset, the separable patch sums and the values' loads execute as the device executes them. Built by
// tests/_guided_ref.py. Includes emu_guide.cpp for its `prepare` (emu_denoise.cpp's) and for k_dn_filter_halves.
#include "emu_guide.cpp"
#include "../../tray_rust_amd/csrc/hip/guided_kernels.h"

using namespace tr_guided;

// one k_gdn_filter<patch> launch as guided.hip makes it
static int guided_filter(const float4* guide, const float4* values, uint32_t width, uint32_t height, uint32_t radius, uint32_t patch, float k, float4* out4) {
    return dn_with_patch(patch, [&](auto f) {
        constexpr int F = decltype(f)::value;
        return hip_emu::launch_simt(dn_tiles_x(width) * dn_tiles_y(height), DN_BLOCK, [&] { k_gdn_filter<F>(guide, values, width, height, radius, k, out4); });
    });
}

static bool bad_args(uint32_t width, uint32_t height, uint32_t radius, uint32_t patch) {
    return width == 0u || height == 0u || radius < 1u || radius > DN_RMAX || patch > DN_FMAX;
}

extern "C" {

uint64_t emu_guided_scratch_bytes(uint32_t width, uint32_t height) { return gdn_scratch_bytes(width, height); }
uint64_t emu_two_pass_scratch_bytes(uint32_t width, uint32_t height) { return gdn_two_pass_scratch_bytes(width, height); }

// the five launches of one tray_denoise_guided_device call, in its order and with its scratch layout (guided.hip: layout)
int emu_denoise_guided(uint32_t width, uint32_t height, const float* even, const float* odd, const float* guide_a, const float* guide_b, uint32_t radius,
                       uint32_t patch, float k, float* out, void* scratch) {
    if (bad_args(width, height, radius, patch)) return -2;
    const size_t n = (size_t)width * height;
    float4* const values = static_cast<float4*>(scratch);
    float4* const guide = values + 3u * n;
    int rc = prepare(reinterpret_cast<const float4*>(even), reinterpret_cast<const float4*>(odd), width, height, values);
    if (rc == 0) rc = prepare(reinterpret_cast<const float4*>(guide_a), reinterpret_cast<const float4*>(guide_b), width, height, guide);
    if (rc == 0) rc = guided_filter(guide, values, width, height, radius, patch, k, reinterpret_cast<float4*>(out));
    return rc;
}

// the six launches of one tray_denoise_two_pass_device call, in its order and with its scratch layout (guided.hip: two_pass_layout)
int emu_denoise_two_pass(uint32_t width, uint32_t height, const float* even, const float* odd, uint32_t radius, uint32_t patch, float k, uint32_t radius2,
                         uint32_t patch2, float k2, float* out, void* scratch) {
    if (bad_args(width, height, radius, patch) || bad_args(width, height, radius2, patch2)) return -2;
    const size_t n = (size_t)width * height;
    float4* const values = static_cast<float4*>(scratch);
    float4* const fa = values + 3u * n;
    float4* const fb = values + 4u * n;
    float4* const guide = values + 5u * n;
    int rc = prepare(reinterpret_cast<const float4*>(even), reinterpret_cast<const float4*>(odd), width, height, values);
    if (rc == 0)
        rc = dn_with_patch(patch, [&](auto f) {
            constexpr int F = decltype(f)::value;
            return hip_emu::launch_simt(dn_tiles_x(width) * dn_tiles_y(height), DN_BLOCK,
                                        [&] { k_dn_filter_halves<F>(values, width, height, radius, k, nullptr, fa, fb); });
        });
    if (rc == 0) rc = prepare(fa, fb, width, height, guide);
    if (rc == 0) rc = guided_filter(guide, values, width, height, radius2, patch2, k2, reinterpret_cast<float4*>(out));
    return rc;
}

}  // extern "C"
