// Host emulation of the kernels of tray_denoise_temporal_demodulated_halves_device, tray_denoise_temporal_demodulated_guided_device and
// tray_denoise_temporal_demodulated_two_pass_device (tray_rust_amd/csrc/hip/td2pass_kernels.h): k_tdm_prepare, k_dn_prepare, k_t2p_halves_pass,
// k_dn_filter_halves and k_td2_guided_pass, compiled by g++ behind hip_emu.h and run as SIMT fibers, as tests/emu/emu_temporal2.cpp runs the
// two-pass temporal call's. Built by tests/_td2pass_ref.py. Includes emu_temporal2.cpp for its `prepare`, `halves_pass` and k_dn_filter_halves.
#include "emu_temporal2.cpp"
#include "../../tray_rust_amd/csrc/hip/td2pass_kernels.h"

using namespace tr_td2pass;

// the two preparing launches of one frame's values as td2pass.hip makes them
static int prepare_demodulated(const float* even, const float* odd, const float* albedo, uint32_t width, uint32_t height, float4* records) {
    const uint32_t blocks = (uint32_t)(((uint64_t)width * height + DN_PREP_BLOCK - 1u) / DN_PREP_BLOCK);
    const float4* const e4 = f4(even);
    const float4* const o4 = f4(odd);
    const float4* const a4 = f4(albedo);
    const int rc = hip_emu::launch_simt(blocks, DN_PREP_BLOCK, [&] { k_tdm_prepare(e4, o4, a4, width, height, records); });
    return rc != 0 ? rc : hip_emu::launch_simt(blocks, DN_PREP_BLOCK, [&] { k_dn_prepare<1>(e4, o4, width, height, records); });
}

// one k_td2_guided_pass<patch> launch as td2pass.hip makes it
static int guided_pass_scaled(const float4* centre_guide, const float4* guide, const float4* values, const float4* albedo, uint32_t width, uint32_t height,
                              uint32_t radius, uint32_t patch, float k, float4* sums, uint32_t first, uint32_t last, float4* out) {
    return dn_with_patch(patch, [&](auto f) {
        constexpr int F = decltype(f)::value;
        return hip_emu::launch_simt(dn_tiles_x(width) * dn_tiles_y(height), DN_BLOCK,
                                    [&] { k_td2_guided_pass<F>(centre_guide, guide, values, albedo, width, height, radius, k, sums, first, last, out); });
    });
}

// the 3 (N + 1) launches of the pilot over all frames' demodulated films, as device_api.hip's demodulated_halves_launches
static int demodulated_halves(uint32_t width, uint32_t height, const float* even, const float* odd, const float* albedo, uint32_t n_neighbours,
                              const float* const* nb_even, const float* const* nb_odd, const float* const* nb_albedo, uint32_t radius, uint32_t radius_t,
                              uint32_t patch, float k, float4* fa, float4* fb, float4* centre, float4* neighbour, float4* sums) {
    int rc = prepare_demodulated(even, odd, albedo, width, height, centre);
    if (rc == 0) rc = halves_pass(centre, centre, width, height, radius, patch, k, sums, 1u, n_neighbours == 0u ? 1u : 0u, fa, fb);
    for (uint32_t j = 0; j < n_neighbours && rc == 0; ++j) {
        rc = prepare_demodulated(nb_even[j], nb_odd[j], nb_albedo[j], width, height, neighbour);
        if (rc == 0) rc = halves_pass(centre, neighbour, width, height, radius_t, patch, k, sums, 0u, j + 1u == n_neighbours ? 1u : 0u, fa, fb);
    }
    return rc;
}

extern "C" {

uint64_t emu_td2_halves_scratch_bytes(uint32_t width, uint32_t height) { return td2_halves_scratch_bytes(width, height); }
uint64_t emu_td2_guided_scratch_bytes(uint32_t width, uint32_t height) { return td2_guided_scratch_bytes(width, height); }
uint64_t emu_td2_two_pass_scratch_bytes(uint32_t width, uint32_t height) { return td2_two_pass_scratch_bytes(width, height); }

// one tray_denoise_temporal_demodulated_halves_device call, in its order and with its scratch layout (t2pass.hip: halves_layout)
int emu_td2_halves(uint32_t width, uint32_t height, const float* even, const float* odd, const float* albedo, uint32_t n_neighbours,
                   const float* const* nb_even, const float* const* nb_odd, const float* const* nb_albedo, uint32_t radius, uint32_t radius_t, uint32_t patch,
                   float k, float* fa, float* fb, void* scratch) {
    if (bad_args(width, height, radius, radius_t, patch)) return -2;
    const size_t n = (size_t)width * height;
    float4* const centre = static_cast<float4*>(scratch);
    return demodulated_halves(width, height, even, odd, albedo, n_neighbours, nb_even, nb_odd, nb_albedo, radius, radius_t, patch, k,
                              reinterpret_cast<float4*>(fa), reinterpret_cast<float4*>(fb), centre, centre + 3u * n, centre + 6u * n);
}

// the 5 (N + 1) launches of one tray_denoise_temporal_demodulated_guided_device call, in its order and with its scratch layout (guided_layout)
int emu_td2_guided(uint32_t width, uint32_t height, const float* even, const float* odd, const float* albedo, const float* guide_a, const float* guide_b,
                   uint32_t n_neighbours, const float* const* nb_even, const float* const* nb_odd, const float* const* nb_albedo,
                   const float* const* nb_guide_a, const float* const* nb_guide_b, uint32_t radius, uint32_t radius_t, uint32_t patch, float k, float* out,
                   void* scratch) {
    if (bad_args(width, height, radius, radius_t, patch)) return -2;
    const size_t n = (size_t)width * height;
    float4* const centre_guide = static_cast<float4*>(scratch);
    float4* const guide = centre_guide + 3u * n;
    float4* const values = centre_guide + 6u * n;
    float4* const sums = centre_guide + 9u * n;
    float4* const out4 = reinterpret_cast<float4*>(out);
    const float4* const alb0 = f4(albedo);
    int rc = prepare_demodulated(even, odd, albedo, width, height, values);
    if (rc == 0) rc = prepare(f4(guide_a), f4(guide_b), width, height, centre_guide);
    if (rc == 0) rc = guided_pass_scaled(centre_guide, centre_guide, values, alb0, width, height, radius, patch, k, sums, 1u, n_neighbours == 0u ? 1u : 0u, out4);
    for (uint32_t j = 0; j < n_neighbours && rc == 0; ++j) {
        rc = prepare_demodulated(nb_even[j], nb_odd[j], nb_albedo[j], width, height, values);
        if (rc == 0) rc = prepare(f4(nb_guide_a[j]), f4(nb_guide_b[j]), width, height, guide);
        if (rc == 0)
            rc = guided_pass_scaled(centre_guide, guide, values, alb0, width, height, radius_t, patch, k, sums, 0u, j + 1u == n_neighbours ? 1u : 0u, out4);
    }
    return rc;
}

// the 9 N + 6 launches of one tray_denoise_temporal_demodulated_two_pass_device call, in its order and with its scratch layout (two_pass_layout)
int emu_td2_two_pass(uint32_t width, uint32_t height, const float* even, const float* odd, const float* albedo, uint32_t n_neighbours,
                     const float* const* nb_even, const float* const* nb_odd, const float* const* nb_albedo, uint32_t radius, uint32_t radius_t,
                     uint32_t patch, float k, uint32_t radius2, uint32_t radius_t2, uint32_t patch2, float k2, float* out, void* scratch) {
    if (bad_args(width, height, radius, radius_t, patch) || bad_args(width, height, radius2, radius_t2, patch2)) return -2;
    const size_t n = (size_t)width * height;
    float4* const centre = static_cast<float4*>(scratch);
    float4* const neighbour = centre + 3u * n;
    float4* const sums = centre + 6u * n;
    float4* const fa = centre + 8u * n;
    float4* const fb = centre + 9u * n;
    float4* const centre_guide = centre + 10u * n;
    float4* const guide = centre + 13u * n;
    float4* const out4 = reinterpret_cast<float4*>(out);
    const float4* const alb0 = f4(albedo);
    const uint32_t grid = dn_tiles_x(width) * dn_tiles_y(height);
    int rc = demodulated_halves(width, height, even, odd, albedo, n_neighbours, nb_even, nb_odd, nb_albedo, radius, radius_t, patch, k, fa, fb, centre,
                                neighbour, sums);
    if (rc == 0) rc = prepare(fa, fb, width, height, centre_guide);
    if (rc == 0) rc = guided_pass_scaled(centre_guide, centre_guide, centre, alb0, width, height, radius2, patch2, k2, sums, 1u, n_neighbours == 0u ? 1u : 0u, out4);
    for (uint32_t j = 0; j < n_neighbours && rc == 0; ++j) {
        rc = prepare_demodulated(nb_even[j], nb_odd[j], nb_albedo[j], width, height, neighbour);
        if (rc == 0)
            rc = dn_with_patch(patch, [&](auto f) {
                constexpr int F = decltype(f)::value;
                return hip_emu::launch_simt(grid, DN_BLOCK, [&] { k_dn_filter_halves<F>(neighbour, width, height, radius, k, nullptr, fa, fb); });
            });
        if (rc == 0) rc = prepare(fa, fb, width, height, guide);
        if (rc == 0)
            rc = guided_pass_scaled(centre_guide, guide, neighbour, alb0, width, height, radius_t2, patch2, k2, sums, 0u, j + 1u == n_neighbours ? 1u : 0u, out4);
    }
    return rc;
}

}  // extern "C"
