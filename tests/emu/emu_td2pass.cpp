// Host emulation of the kernels of tray_denoise_temporal_demodulated_halves_device, tray_denoise_temporal_demodulated_guided_device and
// tray_denoise_temporal_demodulated_two_pass_device (tray_rust_amd/csrc/hip/td2pass_kernels.h): k_tdm_prepare, k_dn_prepare, k_t2p_halves_pass,
// k_dn_filter_halves and k_td2_guided_pass, compiled by g++ behind hip_emu.h and run as SIMT fibers, as tests/emu/emu_temporal2.cpp runs the
// two-pass temporal call's. Built by tests/_td2pass_ref.py. Includes emu_temporal2.cpp for T2Ops (EmuOps, k_dn_filter_halves and k_t2p_halves_pass).
// Also exports denoise_plan.h's layouts and launch counts by number (denoise_plan_record.h) for tests/test_denoise_plan.py.
#include "emu_temporal2.cpp"
#include "../../tray_rust_amd/csrc/hip/td2pass_kernels.h"
#include "denoise_plan_record.h"

using namespace tr_td2pass;

struct Td2Ops : T2Ops {
    using T2Ops::T2Ops;
    // the two preparing launches of one frame's values as td2pass.hip makes them
    void td2_prepare(const float* even, const float* odd, const float* albedo, void* records) {
        const float4* const e4 = emu_f4(even), * const o4 = emu_f4(odd), * const a4 = emu_f4(albedo);
        float4* const s4 = emu_f4(records);
        const uint32_t blocks = (uint32_t)(((uint64_t)width * height + DN_PREP_BLOCK - 1u) / DN_PREP_BLOCK);
        run(blocks, DN_PREP_BLOCK, [&] { k_tdm_prepare(e4, o4, a4, width, height, s4); });
        run(blocks, DN_PREP_BLOCK, [&] { k_dn_prepare<1>(e4, o4, width, height, s4); });
    }
    // one k_td2_guided_pass<patch> launch as td2pass.hip makes it
    void td2_guided_pass(const void* centre_guide, const void* guide, const void* values, const float* albedo, uint32_t radius, uint32_t patch, float k,
                         void* sums, bool first, bool last, float* out) {
        const float4* const c4 = emu_f4(centre_guide), * const g4 = emu_f4(guide), * const v4 = emu_f4(values), * const a4 = emu_f4(albedo);
        float4* const acc4 = emu_f4(sums), * const out4 = emu_f4(out);
        run_tiles(patch, [&](auto f) {
            k_td2_guided_pass<decltype(f)::value>(c4, g4, v4, a4, width, height, radius, k, acc4, first ? 1u : 0u, last ? 1u : 0u, out4);
        });
    }
};

extern "C" {

uint64_t emu_td2_halves_scratch_bytes(uint32_t width, uint32_t height) { return td2_halves_scratch_bytes(width, height); }
uint64_t emu_td2_guided_scratch_bytes(uint32_t width, uint32_t height) { return td2_guided_scratch_bytes(width, height); }
uint64_t emu_td2_two_pass_scratch_bytes(uint32_t width, uint32_t height) { return td2_two_pass_scratch_bytes(width, height); }

// one tray_denoise_temporal_demodulated_halves_device call: the plan's schedule (3 (N + 1) launches) and scratch layout
int emu_td2_halves(uint32_t width, uint32_t height, const float* even, const float* odd, const float* albedo, uint32_t n_neighbours,
                   const float* const* nb_even, const float* const* nb_odd, const float* const* nb_albedo, uint32_t radius, uint32_t radius_t, uint32_t patch,
                   float k, float* fa, float* fb, void* scratch) {
    const dn::Params p{radius, radius_t, patch, k};
    if (emu_refused(emu_temporal_args(width, height, n_neighbours, p))) return -2;
    Td2Ops ops(width, height);
    dn::temporal_demodulated_halves(ops, dn::Frame{even, odd, albedo, nullptr, nullptr}, dn::Neighbours{n_neighbours, nb_even, nb_odd, nb_albedo, nullptr, nullptr},
                                    p, fa, fb, scratch);
    return ops.rc;
}

// one tray_denoise_temporal_demodulated_guided_device call: the plan's schedule (5 (N + 1) launches) and scratch layout
int emu_td2_guided(uint32_t width, uint32_t height, const float* even, const float* odd, const float* albedo, const float* guide_a, const float* guide_b,
                   uint32_t n_neighbours, const float* const* nb_even, const float* const* nb_odd, const float* const* nb_albedo,
                   const float* const* nb_guide_a, const float* const* nb_guide_b, uint32_t radius, uint32_t radius_t, uint32_t patch, float k, float* out,
                   void* scratch) {
    const dn::Params p{radius, radius_t, patch, k};
    if (emu_refused(emu_temporal_args(width, height, n_neighbours, p))) return -2;
    Td2Ops ops(width, height);
    dn::temporal_demodulated_guided(ops, dn::Frame{even, odd, albedo, guide_a, guide_b},
                                    dn::Neighbours{n_neighbours, nb_even, nb_odd, nb_albedo, nb_guide_a, nb_guide_b}, p, out, scratch);
    return ops.rc;
}

// one tray_denoise_temporal_demodulated_two_pass_device call: the plan's schedule (9 N + 6 launches) and scratch layout
int emu_td2_two_pass(uint32_t width, uint32_t height, const float* even, const float* odd, const float* albedo, uint32_t n_neighbours,
                     const float* const* nb_even, const float* const* nb_odd, const float* const* nb_albedo, uint32_t radius, uint32_t radius_t,
                     uint32_t patch, float k, uint32_t radius2, uint32_t radius_t2, uint32_t patch2, float k2, float* out, void* scratch) {
    const dn::Params p{radius, radius_t, patch, k}, second{radius2, radius_t2, patch2, k2};
    if (emu_refused(emu_temporal_args(width, height, n_neighbours, p)) || emu_refused(emu_temporal_args(width, height, n_neighbours, second))) return -2;
    Td2Ops ops(width, height);
    dn::temporal_demodulated_two_pass(ops, dn::Frame{even, odd, albedo, nullptr, nullptr},
                                      dn::Neighbours{n_neighbours, nb_even, nb_odd, nb_albedo, nullptr, nullptr}, p, second, out, scratch);
    return ops.rc;
}

// denoise_plan.h by number (dn_record::Call): the layout's regions as (offset, bytes) pairs into regions[0, 2 * capacity) and its total into *total,
// returns the number of regions; the launches the schedule makes with n neighbours
uint32_t emu_denoise_plan_layout(uint32_t call, uint32_t width, uint32_t height, uint64_t* regions, uint32_t capacity, uint64_t* total) {
    const dn_record::Regions l = dn_record::layout(call, width, height);
    for (size_t i = 0; i < l.regions.size() && i < capacity; ++i) { regions[2 * i] = l.regions[i].offset; regions[2 * i + 1] = l.regions[i].bytes; }
    *total = l.total;
    return (uint32_t)l.regions.size();
}
uint32_t emu_denoise_plan_launches(uint32_t call, uint32_t n) { return dn_record::record(call, n).launches; }

}  // extern "C"
