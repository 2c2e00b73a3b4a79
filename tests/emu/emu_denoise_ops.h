// The host emulation's side of tray_rust_amd/csrc/hip/denoise_plan.h: the plan's schedules run here with an Ops whose members launch the kernels as
// SIMT fibers, where device_api.hip's forward to the add-on libraries -- so the order of the launches, the scratch offsets and the parameter rules
// of an emulated call are the library's by construction. EmuOps holds what every emulation library compiles (k_dn_prepare, k_dn_filter); a member
// names its kernel, so the members of the other groups sit next to their kernels' headers, one layer per emu_*.cpp on top of this one (GuideOps,
// GuidedOps, TemporalOps, TdemodOps, T2Ops, Td2Ops). The first non-zero fiber return is latched in rc and nothing is launched after it.
#pragma once
#include "hip_emu.h"
#include "../../tray_rust_amd/csrc/hip/denoise_kernels.h"
#include "../../tray_rust_amd/csrc/hip/denoise_plan.h"

using namespace tr_denoise;
namespace dn = tr_dnplan;

static_assert(DN_RMAX == 10u && DN_FMAX == 3u, "tr_dnplan::filter_args states the kernels' limits");

// What an emulated call refuses, with -2: the plan's parameter rules. (Its buffer rules are the device's: a test's guarded views of numpy arrays
// need not be 16-byte aligned.)
inline bool emu_refused(const dn::Refusal& no) { return no.rc != TRAY_OK; }
inline dn::Refusal emu_filter_args(uint32_t width, uint32_t height, const dn::Params& p) { return dn::filter_args("", width, height, p.radius, p.patch, p.k); }
inline dn::Refusal emu_temporal_args(uint32_t width, uint32_t height, uint32_t n, const dn::Params& p) {
    return dn::temporal_args("", width, height, n, p.radius, p.radius_t, p.patch, p.k);
}

inline const float4* emu_f4(const void* p) { return static_cast<const float4*>(p); }
inline float4* emu_f4(void* p) { return static_cast<float4*>(p); }

struct EmuOps {
    uint32_t width, height;
    int rc = 0;
    EmuOps(uint32_t w, uint32_t h) : width(w), height(h) {}
    template <class K>
    void run(uint32_t blocks, uint32_t threads, K&& kernel) {
        if (rc == 0) rc = hip_emu::launch_simt(blocks, threads, kernel);
    }
    // one launch over all 32 x 16 tiles of the kernel that body(F) runs, F the patch radius as a constant
    template <class Body>
    void run_tiles(uint32_t patch, Body&& body) { run_tiles(dn_tiles_x(width) * dn_tiles_y(height), patch, body); }
    template <class Body>
    void run_tiles(uint32_t grid, uint32_t patch, Body&& body) {
        dn_with_patch(patch, [&](auto f) { run(grid, DN_BLOCK, [&] { body(f); }); });
    }
    // the two k_dn_prepare launches of tr_denoise::prepare (denoise.hip), in its order
    void prepare(const float* even, const float* odd, void* records) {
        const float4* const e4 = emu_f4(even), * const o4 = emu_f4(odd);
        float4* const s4 = emu_f4(records);
        const uint32_t blocks = (uint32_t)(((uint64_t)width * height + DN_PREP_BLOCK - 1u) / DN_PREP_BLOCK);
        run(blocks, DN_PREP_BLOCK, [&] { k_dn_prepare<0>(e4, o4, width, height, s4); });
        run(blocks, DN_PREP_BLOCK, [&] { k_dn_prepare<1>(e4, o4, width, height, s4); });
    }
    // the three launches of tr_denoise::denoise (denoise.hip), in its order
    void denoise(const float* even, const float* odd, uint32_t radius, uint32_t patch, float k, float* out, void* scratch) {
        prepare(even, odd, scratch);
        const float4* const s4 = emu_f4(scratch);
        float4* const out4 = emu_f4(out);
        run_tiles(patch, [&](auto f) { k_dn_filter<decltype(f)::value>(s4, width, height, radius, k, out4); });
    }
};
