// TEST INFRASTRUCTURE ONLY: a stand-alone program that runs the host-only functions of csrc/hip/noise_plan.h -- the two layouts at several sizes, with the
// last byte of every region written into vectors of the plan's sizes; the schedule of both rules with a recording Ops for scripted count reads, to
// "no tile left", to max_spp and into both refusals; the rules on good and bad argument sets -- to be built with the host sanitizers and run by hand
// on a machine without a GPU (no test runs it):
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/noise_plan_check noise_plan_check.cpp && /tmp/noise_plan_check
// Exit status 0: every layout is packed and aligned, every schedule makes the launches the plan's counts state and ends as expected, every argument
// set is judged as expected, and no sanitizer report.
#include <cstdio>
#include <utility>

#include "noise_plan_record.h"

namespace {
namespace nt = tr_ntplan;
using namespace nt_record;

int walk(const char* what, std::initializer_list<nt::Region> regions, uint64_t total, const uint64_t* align, bool touch) {
    int bad = 0;
    std::vector<unsigned char> buf(touch ? total : 0u);
    uint64_t end = 0;
    size_t i = 0;
    for (const nt::Region& r : regions) {
        bad += r.offset != end || r.bytes == 0u || (r.offset % align[i++]) != 0u;
        end = r.offset + r.bytes;
        if (touch) { buf[r.offset] = 1u; buf[end - 1u] = 1u; }
    }
    bad += end != total;
    if (bad) std::printf("WRONG layout %s\n", what);
    return bad;
}

int expect(const char* what, const nt::Refusal& got, int rc, const char* msg) {
    const bool bad = got.rc != rc || got.msg != msg;
    if (bad) std::printf("WRONG %s: %d \"%s\", expected %d \"%s\"\n", what, got.rc, got.msg.c_str(), rc, msg);
    return bad;
}

// one scripted schedule over 48 tiles of a 64 x 48 frame: the return code, the number of rounds (by their error launches) and the launch count
int run(const char* what, bool filtered, bool with_out, uint32_t lo, uint32_t hi, std::initializer_list<uint32_t> script, int rc, uint32_t rounds) {
    const std::vector<uint32_t> words(script);
    const Recorded r = record(filtered, with_out, 64u, 48u, 48u, 48u, lo, hi, 1u, words.data(), (uint32_t)words.size());
    uint32_t errors = 0, unknown = 0;
    for (const Row& row : r.rows) {
        errors += row.w[0] == kError;
        for (uint32_t i = 1; i < kRowWords; ++i) unknown += (row.w[i] >> 56) == kUnknown;   // (a pointer outside every buffer of the call)
    }
    const bool bad = r.rc != rc || errors != rounds || unknown != 0u || (rc == TRAY_OK && r.launches != nt::call_launches(filtered, with_out, rounds, 1u));
    std::printf("%-44s rc %d, %u rounds, %u launches in %zu groups%s\n", what, r.rc, errors, r.launches, r.rows.size(), bad ? " WRONG" : "");
    return bad;
}

}  // namespace

int main() {
    int bad = 0;
    const uint64_t tile_align[] = {8u, 4u, 4u, 4u, 4u, 4u}, film_align[] = {16u, 16u, 16u, 4u, 4u, 4u};
    for (uint32_t n : {1u, 48u, 32400u, 400000000u}) {
        const nt::TileLayout l = nt::tile_layout(n);
        bad += walk("tiles", {l.list, l.list_q, l.active, l.samples, l.err, l.count}, l.total, tile_align, n < 100000u);
        bad += l.total != (uint64_t)n * 24u + 4u;
    }
    for (auto [w, h] : {std::pair<uint32_t, uint32_t>{1u, 1u}, {33u, 17u}, {64u, 48u}, {1920u, 1080u}, {65535u, 65535u}}) {
        const nt::FilteredLayout l = nt::filtered_layout(w, h);
        bad += walk("filtered", {l.records, l.fa, l.fb, l.flags, l.list, l.counts}, l.total, film_align, w < 2000u);
        bad += l.total != (uint64_t)w * h * 80u + (uint64_t)((w + 31u) / 32u) * ((h + 15u) / 16u) * 8u + 16u || l.total != nt::filtered_scratch_bytes(w, h);
    }
    bad += nt::filtered_scratch_bytes(0u, 7u) != 0u || nt::filtered_scratch_bytes(7u, 0u) != 0u;

    for (bool filtered : {false, true})
        for (bool with_out : {false, true}) {
            if (!filtered && with_out) continue;   // (the raw rule has no output)
            const char* const rule = filtered ? (with_out ? "filtered, out" : "filtered") : "raw";
            std::printf("%s\n", rule);
            // (the filtered rule reads the first block count, then (tiles, blocks) per round; the raw rule the tiles alone)
            if (filtered) {
                bad += run("  48 -> 10 -> 3 -> 0", true, with_out, 8u, 64u, {6u, 10u, 4u, 3u, 2u, 0u, 0u}, TRAY_OK, 3u);
                bad += run("  never empty: ends at max_spp", true, with_out, 8u, 64u, {6u, 48u, 6u, 48u, 6u, 48u, 6u, 48u, 6u}, TRAY_OK, 4u);
                bad += run("  min_spp == max_spp", true, with_out, 16u, 16u, {6u, 0u, 0u}, TRAY_OK, 1u);
                bad += run("  a list longer than the queue", true, with_out, 8u, 64u, {6u, 49u, 6u}, TRAY_E_DEVICE, 1u);
                bad += run("  more blocks than the frame has, at once", true, with_out, 8u, 64u, {7u}, TRAY_E_DEVICE, 0u);
                bad += run("  more blocks than the frame has, later", true, with_out, 8u, 64u, {6u, 10u, 7u}, TRAY_E_DEVICE, 1u);
            } else {
                bad += run("  48 -> 10 -> 3 -> 0", false, with_out, 8u, 64u, {10u, 3u, 0u}, TRAY_OK, 3u);
                bad += run("  never empty: ends at max_spp", false, with_out, 8u, 64u, {48u, 48u, 48u, 48u}, TRAY_OK, 4u);
                bad += run("  min_spp == max_spp", false, with_out, 16u, 16u, {0u}, TRAY_OK, 1u);
                bad += run("  a list longer than the queue", false, with_out, 8u, 64u, {49u}, TRAY_E_DEVICE, 1u);
            }
        }

    // the rules: 16-byte aligned stand-ins for device buffers, never followed
    alignas(16) static float buf[6][8];
    const nt::Scene s{true, TRAY_SAMPLER_LOW_DISCREPANCY, false, 64u, 48u};
    const char* const who = "call";
    bad += expect("raw", nt::target_rules(who, s, 8u, 64u, 0.05f, buf[0], buf[1], buf[2], buf[3]), TRAY_OK, "");
    bad += expect("raw: no scene", nt::target_rules(who, nt::Scene{false, 0u, false, 0u, 0u}, 8u, 64u, 0.05f, buf[0], buf[1], buf[2], buf[3]), TRAY_E_INVALID,
                  "call: null argument");
    bad += expect("raw: min_spp 1", nt::target_rules(who, s, 1u, 64u, 0.05f, buf[0], buf[1], buf[2], buf[3]), TRAY_E_INVALID,
                  "call: min_spp and max_spp must be powers of two with 2 <= min_spp <= max_spp");
    bad += expect("raw: NaN", nt::target_rules(who, s, 8u, 64u, std::nanf(""), buf[0], buf[1], buf[2], buf[3]), TRAY_E_INVALID,
                  "call: threshold must be >= 0 (and not NaN)");
    bad += expect("raw: one film twice", nt::target_rules(who, s, 8u, 64u, 0.05f, buf[0], buf[0], buf[2], buf[3]), TRAY_E_INVALID,
                  "call: the even and odd films must be different buffers");
    bad += expect("raw: Adaptive before broken", nt::target_rules(who, nt::Scene{true, TRAY_SAMPLER_ADAPTIVE, true, 64u, 48u}, 8u, 64u, 0.05f, buf[0], buf[1], buf[2], buf[3]),
                  TRAY_E_UNSUPPORTED, "call: sample ranges exist for the LowDiscrepancy sampler only");
    bad += expect("raw: broken", nt::target_rules(who, nt::Scene{true, TRAY_SAMPLER_LOW_DISCREPANCY, true, 64u, 48u}, 8u, 64u, 0.05f, buf[0], buf[1], buf[2], buf[3]),
                  TRAY_E_INVALID, "this device scene is unusable: a tray_scene_update_frame on it failed");
    bad += expect("filtered", nt::filtered_rules(who, s, 8u, 64u, 0.05f, buf[0], buf[1], 7u, 3u, 0.45f, nullptr, buf[4], buf[2], buf[3]), TRAY_OK, "");
    bad += expect("filtered, out", nt::filtered_rules(who, s, 8u, 64u, 0.05f, buf[0], buf[1], 7u, 3u, 0.45f, buf[5], buf[4], buf[2], buf[3]), TRAY_OK, "");
    bad += expect("filtered: no scratch", nt::filtered_rules(who, s, 8u, 64u, 0.05f, buf[0], buf[1], 7u, 3u, 0.45f, buf[5], nullptr, buf[2], buf[3]), TRAY_E_INVALID,
                  "call: null argument");
    bad += expect("filtered: radius before the buffers", nt::filtered_rules(who, s, 8u, 64u, 0.05f, buf[0], buf[1], 11u, 3u, 0.45f, buf[0], buf[4], buf[2], buf[3]),
                  TRAY_E_INVALID, "call: 1 <= radius <= 10 and patch <= 3 are required");
    bad += expect("filtered: out is a film", nt::filtered_rules(who, s, 8u, 64u, 0.05f, buf[0], buf[1], 7u, 3u, 0.45f, buf[0], buf[4], buf[2], buf[3]), TRAY_E_INVALID,
                  "call: the films, the output and the scratch buffer must be different buffers, 16-byte aligned");
    bad += expect("filtered: scratch unaligned", nt::filtered_rules(who, s, 8u, 64u, 0.05f, buf[0], buf[1], 7u, 3u, 0.45f, nullptr, buf[4] + 1, buf[2], buf[3]),
                  TRAY_E_INVALID, "call: the films, the output and the scratch buffer must be different buffers, 16-byte aligned");
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
