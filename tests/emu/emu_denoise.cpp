// Host emulation of the kernels of tray_denoise_device (tray_rust_amd/csrc/hip/denoise_kernels.h): k_dn_prepare and k_dn_filter, compiled by g++
// behind hip_emu.h and run as SIMT fibers, so that the LDS staging, the per-offset barriers and the separable patch sums execute as the
// device executes them. Built by tests/test_denoise_emu.py; emu_guide.cpp includes this file for `prepare`.
#include "hip_emu.h"
#include "../../tray_rust_amd/csrc/hip/denoise_kernels.h"

using namespace tr_denoise;

// the two k_dn_prepare launches of tr_denoise::prepare (denoise.hip), in its order
static int prepare(const float4* e4, const float4* o4, uint32_t width, uint32_t height, float4* s4) {
    const uint32_t blocks = (uint32_t)(((uint64_t)width * height + DN_PREP_BLOCK - 1u) / DN_PREP_BLOCK);
    const int rc = hip_emu::launch_simt(blocks, DN_PREP_BLOCK, [&] { k_dn_prepare<0>(e4, o4, width, height, s4); });
    return rc != 0 ? rc : hip_emu::launch_simt(blocks, DN_PREP_BLOCK, [&] { k_dn_prepare<1>(e4, o4, width, height, s4); });
}

extern "C" {

uint64_t emu_denoise_scratch_bytes(uint32_t width, uint32_t height) { return dn_scratch_bytes(width, height); }

// the three launches of tr_denoise::denoise (denoise.hip), in its order; scratch: emu_denoise_scratch_bytes(width, height) bytes
int emu_denoise(const float* even, const float* odd, uint32_t width, uint32_t height, uint32_t radius, uint32_t patch, float k, float* out, void* scratch) {
    if (width == 0u || height == 0u || radius < 1u || radius > DN_RMAX || patch > DN_FMAX) return -2;
    float4* const s4 = static_cast<float4*>(scratch);
    float4* const out4 = reinterpret_cast<float4*>(out);
    const int rc = prepare(reinterpret_cast<const float4*>(even), reinterpret_cast<const float4*>(odd), width, height, s4);
    if (rc != 0) return rc;
    return dn_with_patch(patch, [&](auto f) {
        constexpr int F = decltype(f)::value;
        return hip_emu::launch_simt(dn_tiles_x(width) * dn_tiles_y(height), DN_BLOCK, [&] { k_dn_filter<F>(s4, width, height, radius, k, out4); });
    });
}

}  // extern "C"
