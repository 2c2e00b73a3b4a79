// Host emulation of the kernels of tray_denoise_temporal_halves_device, tray_denoise_temporal_guided_device and
// tray_denoise_temporal_two_pass_device (tray_rust_amd/csrc/hip/t2pass_kernels.h): k_dn_prepare, k_dn_filter_halves, k_t2p_halves_pass and
// k_t2p_guided_pass, compiled by g++ behind hip_emu.h and run as SIMT fibers, so that the LDS staging of the guides, the two barriers per offset,
// the values' loads and the sums carried from pass to pass execute as the device executes them. Built by tests/_temporal2_ref.py. Includes
// emu_guide.cpp for its `prepare` (emu_denoise.cpp's) and for k_dn_filter_halves.
#include "emu_guide.cpp"
#include "../../tray_rust_amd/csrc/hip/t2pass_kernels.h"

using namespace tr_t2pass;

static const float4* f4(const float* p) { return reinterpret_cast<const float4*>(p); }

static bool bad_args(uint32_t width, uint32_t height, uint32_t radius, uint32_t radius_t, uint32_t patch) {
    return width == 0u || height == 0u || radius < 1u || radius > DN_RMAX || radius_t < 1u || radius_t > radius || patch > DN_FMAX;
}

// one k_t2p_halves_pass<patch> / k_t2p_guided_pass<patch> launch as t2pass.hip makes it
static int halves_pass(const float4* centre, const float4* frame, uint32_t width, uint32_t height, uint32_t radius, uint32_t patch, float k, float4* sums,
                       uint32_t first, uint32_t last, float4* fa, float4* fb) {
    return dn_with_patch(patch, [&](auto f) {
        constexpr int F = decltype(f)::value;
        return hip_emu::launch_simt(dn_tiles_x(width) * dn_tiles_y(height), DN_BLOCK,
                                    [&] { k_t2p_halves_pass<F>(centre, frame, width, height, radius, k, sums, first, last, fa, fb); });
    });
}

static int guided_pass(const float4* centre_guide, const float4* guide, const float4* values, uint32_t width, uint32_t height, uint32_t radius, uint32_t patch,
                       float k, float4* sums, uint32_t first, uint32_t last, float4* out) {
    return dn_with_patch(patch, [&](auto f) {
        constexpr int F = decltype(f)::value;
        return hip_emu::launch_simt(dn_tiles_x(width) * dn_tiles_y(height), DN_BLOCK,
                                    [&] { k_t2p_guided_pass<F>(centre_guide, guide, values, width, height, radius, k, sums, first, last, out); });
    });
}

// the 3 (N + 1) launches of the pilot over all frames, as device_api.hip's temporal_halves_launches
static int temporal_halves(uint32_t width, uint32_t height, const float* even, const float* odd, uint32_t n_neighbours, const float* const* nb_even,
                           const float* const* nb_odd, uint32_t radius, uint32_t radius_t, uint32_t patch, float k, float4* fa, float4* fb, float4* centre,
                           float4* neighbour, float4* sums) {
    int rc = prepare(f4(even), f4(odd), width, height, centre);
    if (rc == 0) rc = halves_pass(centre, centre, width, height, radius, patch, k, sums, 1u, n_neighbours == 0u ? 1u : 0u, fa, fb);
    for (uint32_t j = 0; j < n_neighbours && rc == 0; ++j) {
        rc = prepare(f4(nb_even[j]), f4(nb_odd[j]), width, height, neighbour);
        if (rc == 0) rc = halves_pass(centre, neighbour, width, height, radius_t, patch, k, sums, 0u, j + 1u == n_neighbours ? 1u : 0u, fa, fb);
    }
    return rc;
}

extern "C" {

uint64_t emu_temporal_halves_scratch_bytes(uint32_t width, uint32_t height) { return t2p_halves_scratch_bytes(width, height); }
uint64_t emu_temporal_guided_scratch_bytes(uint32_t width, uint32_t height) { return t2p_guided_scratch_bytes(width, height); }
uint64_t emu_temporal_two_pass_scratch_bytes(uint32_t width, uint32_t height) { return t2p_two_pass_scratch_bytes(width, height); }

// one tray_denoise_temporal_halves_device call, in its order and with its scratch layout (t2pass.hip: halves_layout)
int emu_denoise_temporal_halves(uint32_t width, uint32_t height, const float* even, const float* odd, uint32_t n_neighbours, const float* const* nb_even,
                                const float* const* nb_odd, uint32_t radius, uint32_t radius_t, uint32_t patch, float k, float* fa, float* fb, void* scratch) {
    if (bad_args(width, height, radius, radius_t, patch)) return -2;
    const size_t n = (size_t)width * height;
    float4* const centre = static_cast<float4*>(scratch);
    return temporal_halves(width, height, even, odd, n_neighbours, nb_even, nb_odd, radius, radius_t, patch, k, reinterpret_cast<float4*>(fa),
                           reinterpret_cast<float4*>(fb), centre, centre + 3u * n, centre + 6u * n);
}

// the 5 (N + 1) launches of one tray_denoise_temporal_guided_device call, in its order and with its scratch layout (t2pass.hip: guided_layout)
int emu_denoise_temporal_guided(uint32_t width, uint32_t height, const float* even, const float* odd, const float* guide_a, const float* guide_b,
                                uint32_t n_neighbours, const float* const* nb_even, const float* const* nb_odd, const float* const* nb_guide_a,
                                const float* const* nb_guide_b, uint32_t radius, uint32_t radius_t, uint32_t patch, float k, float* out, void* scratch) {
    if (bad_args(width, height, radius, radius_t, patch)) return -2;
    const size_t n = (size_t)width * height;
    float4* const centre_guide = static_cast<float4*>(scratch);
    float4* const guide = centre_guide + 3u * n;
    float4* const values = centre_guide + 6u * n;
    float4* const sums = centre_guide + 9u * n;
    float4* const out4 = reinterpret_cast<float4*>(out);
    int rc = prepare(f4(even), f4(odd), width, height, values);
    if (rc == 0) rc = prepare(f4(guide_a), f4(guide_b), width, height, centre_guide);
    if (rc == 0) rc = guided_pass(centre_guide, centre_guide, values, width, height, radius, patch, k, sums, 1u, n_neighbours == 0u ? 1u : 0u, out4);
    for (uint32_t j = 0; j < n_neighbours && rc == 0; ++j) {
        rc = prepare(f4(nb_even[j]), f4(nb_odd[j]), width, height, values);
        if (rc == 0) rc = prepare(f4(nb_guide_a[j]), f4(nb_guide_b[j]), width, height, guide);
        if (rc == 0) rc = guided_pass(centre_guide, guide, values, width, height, radius_t, patch, k, sums, 0u, j + 1u == n_neighbours ? 1u : 0u, out4);
    }
    return rc;
}

// the 9 N + 6 launches of one tray_denoise_temporal_two_pass_device call, in its order and with its scratch layout (t2pass.hip: two_pass_layout)
int emu_denoise_temporal_two_pass(uint32_t width, uint32_t height, const float* even, const float* odd, uint32_t n_neighbours, const float* const* nb_even,
                                  const float* const* nb_odd, uint32_t radius, uint32_t radius_t, uint32_t patch, float k, uint32_t radius2, uint32_t radius_t2,
                                  uint32_t patch2, float k2, float* out, void* scratch) {
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
    const uint32_t grid = dn_tiles_x(width) * dn_tiles_y(height);
    int rc = temporal_halves(width, height, even, odd, n_neighbours, nb_even, nb_odd, radius, radius_t, patch, k, fa, fb, centre, neighbour, sums);
    if (rc == 0) rc = prepare(fa, fb, width, height, centre_guide);
    if (rc == 0) rc = guided_pass(centre_guide, centre_guide, centre, width, height, radius2, patch2, k2, sums, 1u, n_neighbours == 0u ? 1u : 0u, out4);
    for (uint32_t j = 0; j < n_neighbours && rc == 0; ++j) {
        rc = prepare(f4(nb_even[j]), f4(nb_odd[j]), width, height, neighbour);
        if (rc == 0)
            rc = dn_with_patch(patch, [&](auto f) {
                constexpr int F = decltype(f)::value;
                return hip_emu::launch_simt(grid, DN_BLOCK, [&] { k_dn_filter_halves<F>(neighbour, width, height, radius, k, nullptr, fa, fb); });
            });
        if (rc == 0) rc = prepare(fa, fb, width, height, guide);
        if (rc == 0) rc = guided_pass(centre_guide, guide, neighbour, width, height, radius_t2, patch2, k2, sums, 0u, j + 1u == n_neighbours ? 1u : 0u, out4);
    }
    return rc;
}

}  // extern "C"
