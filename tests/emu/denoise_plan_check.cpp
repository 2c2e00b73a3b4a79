// TEST INFRASTRUCTURE ONLY: a stand-alone program that runs the host-only functions of csrc/hip/denoise_plan.h -- every schedule for N = 0, 1, 2, 8 with
// a recording Ops, every layout at four sizes, the rules on good and bad argument sets -- to be built with the host sanitizers and run by hand on a
// machine without a GPU (no test runs it):
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/denoise_plan_check denoise_plan_check.cpp && /tmp/denoise_plan_check
// Exit status 0: every call makes the launches it states, every layout is packed and aligned, every argument set is judged as expected, and no
// sanitizer report.
#include <cstdio>
#include <cstring>
#include <utility>

#include "denoise_plan_record.h"

namespace {
namespace dn = tr_dnplan;
using namespace dn_record;

uint32_t expected_launches(uint32_t call, uint32_t n) {
    switch (call) {
        case kDenoise: case kHalves: return dn::kDenoiseLaunches;
        case kGuided: return dn::kGuidedLaunches;
        case kTwoPass: return dn::kTwoPassLaunches;
        case kDemodulated: return dn::kDenoiseLaunches + dn::kDemodLaunches;
        case kDemodulatedTwoPass: return dn::kTwoPassLaunches + dn::kDemodLaunches;
        case kTemporalGuided: case kTemporalDemodulatedGuided: return 5u * (n + 1u);
        case kTemporalTwoPass: case kTemporalDemodulatedTwoPass: return 9u * n + 6u;
        default: return 3u * (n + 1u);
    }
}

int expect(const char* what, const dn::Refusal& got, int rc, const char* msg) {
    const bool bad = got.rc != rc || got.msg != msg;
    if (bad) std::printf("WRONG %s: %d \"%s\", expected %d \"%s\"\n", what, got.rc, got.msg.c_str(), rc, msg);
    return bad;
}

}  // namespace

int main() {
    int bad = 0;
    for (uint32_t call = 0; call < kCalls; ++call) {
        std::printf("%-32s launches", name(call));
        for (uint32_t n : {0u, 1u, 2u, 8u}) {
            if (call < kTemporal && n) continue;   // (the one-frame calls have no neighbours)
            const RecordingOps ops = record(call, n);
            const bool wrong = ops.launches != expected_launches(call, n);
            std::printf("  N=%u: %u in %zu groups%s", n, ops.launches, ops.groups.size(), wrong ? " WRONG" : "");
            bad += wrong;
        }
        std::printf("\n");
        for (auto [w, h] : {std::pair<uint32_t, uint32_t>{1u, 1u}, {33u, 17u}, {70u, 40u}, {65535u, 65535u}}) {
            const Regions l = layout(call, w, h);
            uint64_t end = 0;
            for (const dn::Region& r : l.regions) { bad += r.offset != end || (r.offset & 15u) != 0u || r.bytes == 0u; end = r.offset + r.bytes; }
            bad += end != l.total || l.total % ((uint64_t)w * h) != 0u;
        }
    }
    // the order of a two-pass temporal call with one neighbour, group by group
    const char* const want[] = {"prepare", "t2_halves_pass", "prepare", "t2_halves_pass", "prepare", "t2_guided_pass", "prepare", "halves", "prepare",
                                "t2_guided_pass"};
    const RecordingOps two = record(kTemporalTwoPass, 1u);
    bad += two.groups.size() != sizeof want / sizeof *want;
    for (size_t i = 0; i < two.groups.size() && i < sizeof want / sizeof *want; ++i) bad += std::strcmp(two.groups[i], want[i]) != 0;

    // the rules: 16-byte aligned stand-ins for device buffers, never followed
    alignas(16) static float buf[12][8];
    const float* const nb_even[2] = {buf[4], buf[5]}, * const nb_odd[2] = {buf[6], buf[7]}, * const nb_same[2] = {buf[4], buf[4]}, * const nb_null[2] = {buf[4], nullptr};
    const dn::Params p{7u, 3u, 3u, 0.45f}, second{5u, 3u, 1u, 0.7f};
    const dn::Frame f{buf[0], buf[1], nullptr, nullptr, nullptr};
    bad += expect("denoise", dn::denoise_rules(33u, 17u, buf[0], buf[1], p, buf[2], buf[3]), TRAY_OK, "");
    bad += expect("denoise: scratch is a film", dn::denoise_rules(33u, 17u, buf[0], buf[1], p, buf[2], buf[0]), TRAY_OK, "");
    bad += expect("denoise: out is a film", dn::denoise_rules(33u, 17u, buf[0], buf[1], p, buf[1], buf[3]), TRAY_E_INVALID,
                  "tray_denoise_device: the two films and the output must be three different buffers");
    bad += expect("denoise: unaligned", dn::denoise_rules(33u, 17u, buf[0], buf[1] + 1, p, buf[2], buf[3]), TRAY_E_INVALID,
                  "tray_denoise_device: the films, the output and the scratch buffer must be 16-byte aligned");
    bad += expect("denoise: k", dn::denoise_rules(33u, 17u, buf[0], buf[1], dn::Params{7u, 0u, 3u, 0.0f}, buf[2], buf[3]), TRAY_E_INVALID,
                  "tray_denoise_device: k must be > 0 and finite");
    bad += expect("halves: list too long", dn::halves_rules(33u, 17u, f, p, reinterpret_cast<const uint32_t*>(buf[8]), 5u, 4u, buf[2], buf[3], buf[9]),
                  TRAY_E_INVALID, "tray_denoise_halves_device: the block list is longer than the frame has blocks");
    bad += expect("halves: empty list", dn::halves_rules(33u, 17u, f, p, reinterpret_cast<const uint32_t*>(buf[8]), 0u, 4u, buf[2], buf[3], buf[9]), TRAY_OK, "");
    bad += expect("guided: the films as guide", dn::guided_rules(33u, 17u, dn::Frame{buf[0], buf[1], nullptr, buf[0], buf[1]}, p, buf[2], buf[3]), TRAY_OK, "");
    bad += dn::guided_rules(33u, 17u, dn::Frame{buf[0], buf[1], nullptr, buf[4], buf[4]}, p, buf[2], buf[3]).rc != TRAY_E_INVALID;   // one guide film twice
    bad += expect("two_pass: second radius", dn::two_pass_rules(33u, 17u, f, p, dn::Params{11u, 0u, 1u, 0.7f}, buf[2], buf[3]), TRAY_E_INVALID,
                  "tray_denoise_two_pass_device, second pass: 1 <= radius <= 10 and patch <= 3 are required");
    bad += expect("demodulated: null albedo", dn::demodulated_rules(33u, 17u, f, p, nullptr, buf[2], buf[3]), TRAY_E_INVALID,
                  "tray_denoise_demodulated_device: null argument");
    const dn::Neighbours nb{2u, nb_even, nb_odd, nullptr, nullptr, nullptr};
    bad += expect("temporal", dn::temporal_rules(33u, 17u, f, nb, p, buf[2], buf[3]), TRAY_OK, "");
    bad += expect("temporal: N", dn::temporal_rules(33u, 17u, f, dn::Neighbours{9u, nb_even, nb_odd, nullptr, nullptr, nullptr}, p, buf[2], buf[3]), TRAY_E_INVALID,
                  "tray_denoise_temporal_device: at most 8 neighbouring frames");
    bad += expect("temporal: radius_t", dn::temporal_rules(33u, 17u, f, nb, dn::Params{3u, 4u, 3u, 0.45f}, buf[2], buf[3]), TRAY_E_INVALID,
                  "tray_denoise_temporal_device: 1 <= radius_t <= radius is required");
    bad += expect("temporal: no array", dn::temporal_rules(33u, 17u, f, dn::Neighbours{2u, nb_even, nullptr, nullptr, nullptr, nullptr}, p, buf[2], buf[3]),
                  TRAY_E_INVALID, "tray_denoise_temporal_device: null argument");
    bad += expect("temporal: null film", dn::temporal_rules(33u, 17u, f, dn::Neighbours{2u, nb_even, nb_null, nullptr, nullptr, nullptr}, p, buf[2], buf[3]),
                  TRAY_E_INVALID, "tray_denoise_temporal_device: null film of a neighbouring frame");
    bad += expect("temporal: a film twice", dn::temporal_rules(33u, 17u, f, dn::Neighbours{2u, nb_same, nb_odd, nullptr, nullptr, nullptr}, p, buf[2], buf[3]),
                  TRAY_E_INVALID, "tray_denoise_temporal_device: every frame's two films, the output and the scratch buffer must be different buffers, 16-byte aligned");
    bad += expect("temporal_guided: the films as guides",
                  dn::temporal_guided_rules(33u, 17u, dn::Frame{buf[0], buf[1], nullptr, buf[0], buf[1]}, dn::Neighbours{2u, nb_even, nb_odd, nullptr, nb_even, nb_odd}, p,
                                            buf[2], buf[3]),
                  TRAY_OK, "");
    bad += dn::temporal_guided_rules(33u, 17u, dn::Frame{buf[0], buf[1], nullptr, buf[0], buf[1]}, dn::Neighbours{2u, nb_even, nb_odd, nullptr, nb_even, nb_odd}, p,
                                     buf[6], buf[3]).rc != TRAY_E_INVALID;   // the output is a neighbour's guide
    bad += expect("temporal_demodulated_guided: the films as guides",
                  dn::temporal_demodulated_guided_rules(33u, 17u, dn::Frame{buf[0], buf[1], buf[10], buf[0], buf[1]}, dn::Neighbours{0u, nullptr, nullptr, nullptr, nullptr, nullptr},
                                                        p, buf[2], buf[3]),
                  TRAY_E_INVALID,
                  "tray_denoise_temporal_demodulated_guided_device: every frame's films and albedo film, the outputs and the scratch buffer must be different "
                  "buffers, 16-byte aligned");
    bad += expect("temporal_two_pass: second radius_t", dn::temporal_two_pass_rules(33u, 17u, f, nb, p, dn::Params{5u, 6u, 1u, 0.7f}, buf[2], buf[3]), TRAY_E_INVALID,
                  "tray_denoise_temporal_two_pass_device, second pass: 1 <= radius_t <= radius is required");
    bad += expect("temporal_two_pass", dn::temporal_two_pass_rules(33u, 17u, f, nb, p, second, buf[2], buf[3]), TRAY_OK, "");
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
