// Host emulation of the kernels of tray_denoise_temporal_device (tray_rust_amd/csrc/hip/temporal_kernels.h): k_dn_prepare and k_tdn_pass, compiled
// by g++ behind hip_emu.h and run as SIMT fibers, so that the LDS staging, the two barriers per offset, the separable patch sums and the sums
// carried from pass to pass execute as the device executes them. Built by tests/_temporal_ref.py. Includes emu_denoise.cpp for EmuOps.
#include "emu_denoise.cpp"
#include "../../tray_rust_amd/csrc/hip/temporal_kernels.h"

using namespace tr_temporal;

static_assert(TDN_RMAX == 10u, "tr_dnplan::filter_args states the kernels' limits");

struct TemporalOps : EmuOps {
    using EmuOps::EmuOps;
    // one k_tdn_pass<patch> launch as temporal.hip makes it
    void temporal_pass(const void* centre, const void* frame, uint32_t radius, uint32_t patch, float k, void* sums, bool first, bool last, float* out) {
        const float4* const c4 = emu_f4(centre), * const f4 = emu_f4(frame);
        float4* const acc4 = emu_f4(sums), * const out4 = emu_f4(out);
        run_tiles(patch, [&](auto f) { k_tdn_pass<decltype(f)::value>(c4, f4, width, height, radius, k, acc4, first ? 1u : 0u, last ? 1u : 0u, out4); });
    }
};

extern "C" {

uint64_t emu_temporal_scratch_bytes(uint32_t width, uint32_t height) { return tdn_scratch_bytes(width, height); }

// one tray_denoise_temporal_device call: the plan's schedule (3 (N + 1) launches) and scratch layout; nb_even / nb_odd: n_neighbours film pointers
// each; scratch: emu_temporal_scratch_bytes(width, height) bytes
int emu_denoise_temporal(uint32_t width, uint32_t height, const float* even, const float* odd, uint32_t n_neighbours, const float* const* nb_even,
                         const float* const* nb_odd, uint32_t radius, uint32_t radius_t, uint32_t patch, float k, float* out, void* scratch) {
    const dn::Params p{radius, radius_t, patch, k};
    if (emu_refused(emu_temporal_args(width, height, n_neighbours, p))) return -2;
    TemporalOps ops(width, height);
    dn::temporal(ops, dn::Frame{even, odd, nullptr, nullptr, nullptr}, dn::Neighbours{n_neighbours, nb_even, nb_odd, nullptr, nullptr, nullptr}, p, out, scratch);
    return ops.rc;
}

}  // extern "C"
