// Host emulation of the kernels of tray_denoise_temporal_halves_device, tray_denoise_temporal_guided_device and
// tray_denoise_temporal_two_pass_device (tray_rust_amd/csrc/hip/t2pass_kernels.h): k_dn_prepare, k_dn_filter_halves, k_t2p_halves_pass and
// k_t2p_guided_pass, compiled by g++ behind hip_emu.h and run as SIMT fibers, so that the LDS staging of the guides, the two barriers per offset,
// the values' loads and the sums carried from pass to pass execute as the device executes them. Built by tests/_temporal2_ref.py. Includes
// emu_guide.cpp for GuideOps (EmuOps and k_dn_filter_halves).
#include "emu_guide.cpp"
#include "../../tray_rust_amd/csrc/hip/t2pass_kernels.h"

using namespace tr_t2pass;

struct T2Ops : GuideOps {
    using GuideOps::GuideOps;
    // one k_t2p_halves_pass<patch> / k_t2p_guided_pass<patch> launch as t2pass.hip makes it
    void t2_halves_pass(const void* centre, const void* frame, uint32_t radius, uint32_t patch, float k, void* sums, bool first, bool last, float* fa, float* fb) {
        const float4* const c4 = emu_f4(centre), * const f4 = emu_f4(frame);
        float4* const acc4 = emu_f4(sums), * const a4 = emu_f4(fa), * const b4 = emu_f4(fb);
        run_tiles(patch, [&](auto f) {
            k_t2p_halves_pass<decltype(f)::value>(c4, f4, width, height, radius, k, acc4, first ? 1u : 0u, last ? 1u : 0u, a4, b4);
        });
    }
    void t2_guided_pass(const void* centre_guide, const void* guide, const void* values, uint32_t radius, uint32_t patch, float k, void* sums, bool first,
                        bool last, float* out) {
        const float4* const c4 = emu_f4(centre_guide), * const g4 = emu_f4(guide), * const v4 = emu_f4(values);
        float4* const acc4 = emu_f4(sums), * const out4 = emu_f4(out);
        run_tiles(patch, [&](auto f) {
            k_t2p_guided_pass<decltype(f)::value>(c4, g4, v4, width, height, radius, k, acc4, first ? 1u : 0u, last ? 1u : 0u, out4);
        });
    }
};

extern "C" {

uint64_t emu_temporal_halves_scratch_bytes(uint32_t width, uint32_t height) { return t2p_halves_scratch_bytes(width, height); }
uint64_t emu_temporal_guided_scratch_bytes(uint32_t width, uint32_t height) { return t2p_guided_scratch_bytes(width, height); }
uint64_t emu_temporal_two_pass_scratch_bytes(uint32_t width, uint32_t height) { return t2p_two_pass_scratch_bytes(width, height); }

// one tray_denoise_temporal_halves_device call: the plan's schedule (3 (N + 1) launches) and scratch layout
int emu_denoise_temporal_halves(uint32_t width, uint32_t height, const float* even, const float* odd, uint32_t n_neighbours, const float* const* nb_even,
                                const float* const* nb_odd, uint32_t radius, uint32_t radius_t, uint32_t patch, float k, float* fa, float* fb, void* scratch) {
    const dn::Params p{radius, radius_t, patch, k};
    if (emu_refused(emu_temporal_args(width, height, n_neighbours, p))) return -2;
    T2Ops ops(width, height);
    dn::temporal_halves(ops, dn::Frame{even, odd, nullptr, nullptr, nullptr}, dn::Neighbours{n_neighbours, nb_even, nb_odd, nullptr, nullptr, nullptr}, p, fa, fb,
                        scratch);
    return ops.rc;
}

// one tray_denoise_temporal_guided_device call: the plan's schedule (5 (N + 1) launches) and scratch layout
int emu_denoise_temporal_guided(uint32_t width, uint32_t height, const float* even, const float* odd, const float* guide_a, const float* guide_b,
                                uint32_t n_neighbours, const float* const* nb_even, const float* const* nb_odd, const float* const* nb_guide_a,
                                const float* const* nb_guide_b, uint32_t radius, uint32_t radius_t, uint32_t patch, float k, float* out, void* scratch) {
    const dn::Params p{radius, radius_t, patch, k};
    if (emu_refused(emu_temporal_args(width, height, n_neighbours, p))) return -2;
    T2Ops ops(width, height);
    dn::temporal_guided(ops, dn::Frame{even, odd, nullptr, guide_a, guide_b}, dn::Neighbours{n_neighbours, nb_even, nb_odd, nullptr, nb_guide_a, nb_guide_b}, p,
                        out, scratch);
    return ops.rc;
}

// one tray_denoise_temporal_two_pass_device call: the plan's schedule (9 N + 6 launches) and scratch layout
int emu_denoise_temporal_two_pass(uint32_t width, uint32_t height, const float* even, const float* odd, uint32_t n_neighbours, const float* const* nb_even,
                                  const float* const* nb_odd, uint32_t radius, uint32_t radius_t, uint32_t patch, float k, uint32_t radius2, uint32_t radius_t2,
                                  uint32_t patch2, float k2, float* out, void* scratch) {
    const dn::Params p{radius, radius_t, patch, k}, second{radius2, radius_t2, patch2, k2};
    if (emu_refused(emu_temporal_args(width, height, n_neighbours, p)) || emu_refused(emu_temporal_args(width, height, n_neighbours, second))) return -2;
    T2Ops ops(width, height);
    dn::temporal_two_pass(ops, dn::Frame{even, odd, nullptr, nullptr, nullptr}, dn::Neighbours{n_neighbours, nb_even, nb_odd, nullptr, nullptr, nullptr}, p,
                          second, out, scratch);
    return ops.rc;
}

}  // extern "C"
