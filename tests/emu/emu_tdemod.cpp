// Host emulation of the kernels of tray_denoise_temporal_demodulated_device (tray_rust_amd/csrc/hip/tdemod_kernels.h): k_tdm_prepare, k_dn_prepare<1>
// and k_tdm_pass, compiled by g++ behind hip_emu.h and run as SIMT fibers, as tests/emu/emu_temporal.cpp runs the temporal call's. Built by
// tests/_tdemod_ref.py.
#include "hip_emu.h"
#include "../../tray_rust_amd/csrc/hip/tdemod_kernels.h"

using namespace tr_tdemod;

extern "C" {

uint64_t emu_tdemod_scratch_bytes(uint32_t width, uint32_t height) { return tdm_scratch_bytes(width, height); }

// the 3 (N + 1) launches of one tray_denoise_temporal_demodulated_device call, in its order and with its scratch layout (tdemod.hip: layout);
// nb_even / nb_odd / nb_albedo: n_neighbours film pointers each; scratch: emu_tdemod_scratch_bytes(width, height) bytes
int emu_denoise_temporal_demodulated(uint32_t width, uint32_t height, const float* even, const float* odd, const float* albedo, uint32_t n_neighbours,
                                     const float* const* nb_even, const float* const* nb_odd, const float* const* nb_albedo, uint32_t radius,
                                     uint32_t radius_t, uint32_t patch, float k, float* out, void* scratch) {
    if (width == 0u || height == 0u || radius < 1u || radius > DN_RMAX || radius_t < 1u || radius_t > radius || patch > DN_FMAX) return -2;
    const size_t n = (size_t)width * height;
    float4* const centre = static_cast<float4*>(scratch);
    float4* const neighbour = centre + 3u * n;
    float4* const sums = centre + 6u * n;
    float4* const out4 = reinterpret_cast<float4*>(out);
    const float4* const alb0 = reinterpret_cast<const float4*>(albedo);
    const uint32_t grid = dn_tiles_x(width) * dn_tiles_y(height);
    const uint32_t blocks = (uint32_t)(((uint64_t)width * height + DN_PREP_BLOCK - 1u) / DN_PREP_BLOCK);
    auto prepare = [&](const float* e, const float* o, const float* a, float4* records) {
        const float4* const e4 = reinterpret_cast<const float4*>(e);
        const float4* const o4 = reinterpret_cast<const float4*>(o);
        const float4* const a4 = reinterpret_cast<const float4*>(a);
        const int rc = hip_emu::launch_simt(blocks, DN_PREP_BLOCK, [&] { k_tdm_prepare(e4, o4, a4, width, height, records); });
        return rc != 0 ? rc : hip_emu::launch_simt(blocks, DN_PREP_BLOCK, [&] { k_dn_prepare<1>(e4, o4, width, height, records); });
    };
    auto pass = [&](const float4* frame, uint32_t r, uint32_t first, uint32_t last) {
        return dn_with_patch(patch, [&](auto f) {
            constexpr int F = decltype(f)::value;
            return hip_emu::launch_simt(grid, DN_BLOCK, [&] { k_tdm_pass<F>(centre, frame, alb0, width, height, r, k, sums, first, last, out4); });
        });
    };
    int rc = prepare(even, odd, albedo, centre);
    if (rc == 0) rc = pass(centre, radius, 1u, n_neighbours == 0u ? 1u : 0u);
    for (uint32_t j = 0; j < n_neighbours && rc == 0; ++j) {
        rc = prepare(nb_even[j], nb_odd[j], nb_albedo[j], neighbour);
        if (rc == 0) rc = pass(neighbour, radius_t, 0u, j + 1u == n_neighbours ? 1u : 0u);
    }
    return rc;
}

}  // extern "C"
