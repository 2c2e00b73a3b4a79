// Host emulation of the kernels of tray_denoise_temporal_demodulated_device (tray_rust_amd/csrc/hip/tdemod_kernels.h): k_tdm_prepare, k_dn_prepare<1>
// and k_tdm_pass, compiled by g++ behind hip_emu.h and run as SIMT fibers, as tests/emu/emu_temporal.cpp runs the temporal call's. Built by
// tests/_tdemod_ref.py.
#include "emu_denoise_ops.h"
#include "../../tray_rust_amd/csrc/hip/tdemod_kernels.h"

using namespace tr_tdemod;

struct TdemodOps : EmuOps {
    using EmuOps::EmuOps;
    // the two preparing launches of one frame as tdemod.hip makes them
    void tdemod_prepare(const float* even, const float* odd, const float* albedo, void* records) {
        const float4* const e4 = emu_f4(even), * const o4 = emu_f4(odd), * const a4 = emu_f4(albedo);
        float4* const s4 = emu_f4(records);
        const uint32_t blocks = (uint32_t)(((uint64_t)width * height + DN_PREP_BLOCK - 1u) / DN_PREP_BLOCK);
        run(blocks, DN_PREP_BLOCK, [&] { k_tdm_prepare(e4, o4, a4, width, height, s4); });
        run(blocks, DN_PREP_BLOCK, [&] { k_dn_prepare<1>(e4, o4, width, height, s4); });
    }
    // one k_tdm_pass<patch> launch as tdemod.hip makes it
    void tdemod_pass(const void* centre, const void* frame, const float* albedo, uint32_t radius, uint32_t patch, float k, void* sums, bool first, bool last,
                     float* out) {
        const float4* const c4 = emu_f4(centre), * const f4 = emu_f4(frame), * const a4 = emu_f4(albedo);
        float4* const acc4 = emu_f4(sums), * const out4 = emu_f4(out);
        run_tiles(patch, [&](auto f) { k_tdm_pass<decltype(f)::value>(c4, f4, a4, width, height, radius, k, acc4, first ? 1u : 0u, last ? 1u : 0u, out4); });
    }
};

extern "C" {

uint64_t emu_tdemod_scratch_bytes(uint32_t width, uint32_t height) { return tdm_scratch_bytes(width, height); }

// one tray_denoise_temporal_demodulated_device call: the plan's schedule (3 (N + 1) launches) and scratch layout; nb_even / nb_odd / nb_albedo:
// n_neighbours film pointers each; scratch: emu_tdemod_scratch_bytes(width, height) bytes
int emu_denoise_temporal_demodulated(uint32_t width, uint32_t height, const float* even, const float* odd, const float* albedo, uint32_t n_neighbours,
                                     const float* const* nb_even, const float* const* nb_odd, const float* const* nb_albedo, uint32_t radius,
                                     uint32_t radius_t, uint32_t patch, float k, float* out, void* scratch) {
    const dn::Params p{radius, radius_t, patch, k};
    if (emu_refused(emu_temporal_args(width, height, n_neighbours, p))) return -2;
    TdemodOps ops(width, height);
    dn::temporal_demodulated(ops, dn::Frame{even, odd, albedo, nullptr, nullptr}, dn::Neighbours{n_neighbours, nb_even, nb_odd, nb_albedo, nullptr, nullptr}, p,
                             out, scratch);
    return ops.rc;
}

}  // extern "C"
