// TEST INFRASTRUCTURE ONLY: tray_rust_amd/csrc/hip/denoise_plan.h's schedules and layouts by number, for tests/test_denoise_plan.py (through
// emu_td2pass.cpp's exports) and for the stand-alone denoise_plan_check.cpp. RecordingOps has every launch group of the plan and launches nothing: it
// notes the group's name and counts the launches the group makes on the device. Needs no kernel header.
#pragma once
#include <cstdint>
#include <vector>

#include "../../tray_rust_amd/csrc/hip/denoise_plan.h"

namespace dn_record {
namespace dn = tr_dnplan;

// the calls, in the order of include/trayhip.h; the demodulated one-frame call once per filter
enum Call : uint32_t {
    kDenoise, kHalves, kGuided, kTwoPass, kDemodulated, kDemodulatedTwoPass, kTemporal, kTemporalDemodulated, kTemporalHalves, kTemporalGuided,
    kTemporalTwoPass, kTemporalDemodulatedHalves, kTemporalDemodulatedGuided, kTemporalDemodulatedTwoPass, kCalls
};
inline const char* name(uint32_t call) {
    static const char* const names[kCalls] = {"denoise", "halves", "guided", "two_pass", "demodulated", "demodulated (two passes)", "temporal",
                                              "temporal_demodulated", "temporal_halves", "temporal_guided", "temporal_two_pass",
                                              "temporal_demodulated_halves", "temporal_demodulated_guided", "temporal_demodulated_two_pass"};
    return call < kCalls ? names[call] : "?";
}

struct RecordingOps {
    uint32_t width, height;
    std::vector<const char*> groups;
    uint32_t launches = 0;
    void note(const char* group, uint32_t n) { groups.push_back(group); launches += n; }
    void prepare(const float*, const float*, void*) { note("prepare", dn::kPrepareLaunches); }
    void denoise(const float*, const float*, uint32_t, uint32_t, float, float*, void*) { note("denoise", dn::kDenoiseLaunches); }
    void halves(const void*, uint32_t, uint32_t, float, const uint32_t*, uint32_t, float*, float*) { note("halves", 1u); }
    void filter(const void*, const void*, uint32_t, uint32_t, float, float*) { note("filter", 1u); }
    void temporal_pass(const void*, const void*, uint32_t, uint32_t, float, void*, bool, bool, float*) { note("temporal_pass", 1u); }
    void tdemod_prepare(const float*, const float*, const float*, void*) { note("tdemod_prepare", dn::kPrepareLaunches); }
    void tdemod_pass(const void*, const void*, const float*, uint32_t, uint32_t, float, void*, bool, bool, float*) { note("tdemod_pass", 1u); }
    void t2_halves_pass(const void*, const void*, uint32_t, uint32_t, float, void*, bool, bool, float*, float*) { note("t2_halves_pass", 1u); }
    void t2_guided_pass(const void*, const void*, const void*, uint32_t, uint32_t, float, void*, bool, bool, float*) { note("t2_guided_pass", 1u); }
    void td2_prepare(const float*, const float*, const float*, void*) { note("td2_prepare", dn::kPrepareLaunches); }
    void td2_guided_pass(const void*, const void*, const void*, const float*, uint32_t, uint32_t, float, void*, bool, bool, float*) {
        note("td2_guided_pass", 1u);
    }
    void demodulate(const float*, const float*, const float*, float*, float*) { note("demodulate", 1u); }
    void remodulate(const float*, float*) { note("remodulate", 1u); }
};

// the schedule of `call` with n neighbours (the one-frame calls take none) over a 1 x 1 frame; no pointer is followed
inline RecordingOps record(uint32_t call, uint32_t n) {
    static float film[4], out[4], fb[4];
    static char scratch[512];
    static const float* const films[TRAY_DENOISE_MAX_NEIGHBOURS] = {film, film, film, film, film, film, film, film};
    const dn::Frame f{film, film, film, film, film};
    const dn::Neighbours nb{n <= TRAY_DENOISE_MAX_NEIGHBOURS ? n : 0u, films, films, films, films, films};
    const dn::Params p{7u, 3u, 3u, 0.45f}, second{5u, 3u, 1u, 0.7f};
    RecordingOps ops{1u, 1u, {}, 0u};
    switch (call) {
        case kDenoise: dn::denoise(ops, f, p, out, scratch); break;
        case kHalves: dn::halves(ops, f, p, nullptr, 0u, out, fb, scratch); break;
        case kGuided: dn::guided(ops, f, p, out, scratch); break;
        case kTwoPass: dn::two_pass(ops, f, p, second, out, scratch); break;
        case kDemodulated: dn::demodulated(ops, f, p, nullptr, out, scratch); break;
        case kDemodulatedTwoPass: dn::demodulated(ops, f, p, &second, out, scratch); break;
        case kTemporal: dn::temporal(ops, f, nb, p, out, scratch); break;
        case kTemporalDemodulated: dn::temporal_demodulated(ops, f, nb, p, out, scratch); break;
        case kTemporalHalves: dn::temporal_halves(ops, f, nb, p, out, fb, scratch); break;
        case kTemporalGuided: dn::temporal_guided(ops, f, nb, p, out, scratch); break;
        case kTemporalTwoPass: dn::temporal_two_pass(ops, f, nb, p, second, out, scratch); break;
        case kTemporalDemodulatedHalves: dn::temporal_demodulated_halves(ops, f, nb, p, out, fb, scratch); break;
        case kTemporalDemodulatedGuided: dn::temporal_demodulated_guided(ops, f, nb, p, out, scratch); break;
        case kTemporalDemodulatedTwoPass: dn::temporal_demodulated_two_pass(ops, f, nb, p, second, out, scratch); break;
        default: break;
    }
    return ops;
}

// the regions of the layout of `call` in the order of its struct, and its total
struct Regions { std::vector<dn::Region> regions; uint64_t total; };
inline Regions layout(uint32_t call, uint32_t w, uint32_t h) {
    switch (call) {
        case kDenoise: case kHalves: { const auto l = dn::plain_layout(w, h); return {{l.records}, l.total}; }
        case kGuided: { const auto l = dn::guided_layout(w, h); return {{l.values, l.guide}, l.total}; }
        case kTwoPass: { const auto l = dn::two_pass_layout(w, h); return {{l.values, l.fa, l.fb, l.guide}, l.total}; }
        case kDemodulated: case kDemodulatedTwoPass: {
            const auto l = dn::demodulated_layout(w, h, call == kDemodulatedTwoPass);
            return {{l.filter, l.even, l.odd}, l.total};
        }
        case kTemporal: case kTemporalDemodulated: case kTemporalHalves: case kTemporalDemodulatedHalves: {
            const auto l = dn::temporal_layout(w, h);
            return {{l.centre, l.neighbour, l.sums}, l.total};
        }
        case kTemporalGuided: case kTemporalDemodulatedGuided: {
            const auto l = dn::temporal_guided_layout(w, h);
            return {{l.centre_guide, l.guide, l.values, l.sums}, l.total};
        }
        case kTemporalTwoPass: case kTemporalDemodulatedTwoPass: {
            const auto l = dn::temporal_two_pass_layout(w, h);
            return {{l.centre, l.neighbour, l.sums, l.fa, l.fb, l.centre_guide, l.guide}, l.total};
        }
        default: return {{}, 0u};
    }
}

}  // namespace dn_record
