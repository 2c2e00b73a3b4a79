// TEST INFRASTRUCTURE ONLY: a stand-alone program that runs csrc/hip/noise_plan.h's schedule with a neighbour bound (include/trayhip.h:
// tray_scene_set_noise_ratio) over scripted Ops -- the per-tile buffers are host memory, a tile's error comes from a table (a noisy tile never
// converges, every other tile converges at once), a render only counts the samples each tile was handed, and the bound's three groups are plain
// C++ statements of the kernels -- and checks where the rounds end. tests/test_nbound_plan.py builds and runs it; it is also what a host-sanitizer
// build compiles and runs:
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -o /tmp/nbound_plan_check nbound_plan_check.cpp && /tmp/nbound_plan_check
// Exit status 0: every case ends at the sample counts stated, every tile was handed exactly [0, n_t) in order, neighbours are within the ratio,
// the launch and read counts are the plan's, a call without a bound makes the unbounded call's groups, and no sanitizer report.
#include <cstdio>
#include <set>
#include <utility>

#include "noise_plan_record.h"

namespace {
namespace nt = tr_ntplan;

struct ScriptedOps {
    uint32_t width, height;
    std::vector<uint32_t> queue;        // (x, y) pairs
    std::set<uint32_t> noisy;           // queue indices whose error never drops
    std::vector<uint32_t> handed;       // per queue index: the samples rendered so far, [0, handed)
    std::vector<uint32_t> groups;       // the launch groups in order (nt_record::Group; the bound's: 100 grid, 101 pull, 102 compact_level)
    std::vector<uint32_t> read_words;   // what every read returned
    uint32_t reads = 0u, bad = 0u;
    std::vector<std::pair<const void*, const uint32_t*>> lists;   // every list a compaction wrote, with its queue indices
    const uint32_t* q_of(const void* list) const {
        for (auto& p : lists) if (p.first == list) return p.second;
        return nullptr;
    }
    int render(const void* list, uint32_t n, uint32_t begin, uint32_t end, float*, uint32_t* launches) {
        groups.push_back(nt_record::kRender);
        const uint32_t* lq = list == queue.data() ? nullptr : q_of(list);
        if (list != queue.data() && !lq) { ++bad; return TRAY_OK; }
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t q = lq ? lq[i] : i;
            if (q >= handed.size() || handed[q] != begin) { ++bad; continue; }   // a range out of order, or twice
            handed[q] = end;
        }
        *launches += 1u;
        return TRAY_OK;
    }
    int block_list(const void*, const uint32_t*, uint32_t, uint32_t*, uint32_t*, uint32_t* count) { groups.push_back(nt_record::kBlockList); *count = 1u; return TRAY_OK; }
    int halves(const float*, const float*, void*, uint32_t, uint32_t, float, const uint32_t*, uint32_t, float*, float*) { groups.push_back(nt_record::kHalves); return TRAY_OK; }
    void error(const float*, const float*, const void* list, const uint32_t* list_q, uint32_t n, uint32_t taken, uint32_t max_spp, float threshold, float* err,
               uint32_t* active, uint32_t* samples) {
        groups.push_back(nt_record::kError);
        (void)list;
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t q = list_q ? list_q[i] : i;
            const float e = noisy.count(q) ? 1.0f : 0.0f;
            if (handed[q] != taken) ++bad;   // the error is taken after the tile's own round
            err[q] = e; samples[q] = taken;
            active[q] = (!(e < threshold) && taken < max_spp) ? 1u : 0u;
        }
    }
    void compact(const void* q, const uint32_t* active, uint32_t n, void* list, uint32_t* list_q, uint32_t* count) {
        groups.push_back(nt_record::kCompact);
        uint32_t o = 0u;
        for (uint32_t i = 0; i < n; ++i)
            if (active[i]) { std::memcpy(static_cast<uint32_t*>(list) + 2u * o, static_cast<const uint32_t*>(q) + 2u * i, 8u); list_q[o++] = i; }
        *count = o;
        lists.push_back({list, list_q});
    }
    int read(const uint32_t* counts, uint32_t n_words, uint32_t* host) {
        groups.push_back(nt_record::kRead);
        ++reads;
        for (uint32_t i = 0; i < n_words; ++i) { host[i] = counts[i]; read_words.push_back(counts[i]); }
        return TRAY_OK;
    }
    int final_filter(const float*, const float*, uint32_t, uint32_t, float, float*, void*) { groups.push_back(nt_record::kFinalFilter); return TRAY_OK; }
    // the bound's groups: host statements of nbound_kernels.h
    int grid(const void* q, uint32_t n, uint32_t* map) {
        groups.push_back(100u);
        const uint32_t gw = nt::grid_w(width), gh = nt::grid_h(height);
        for (uint32_t c = 0; c < gw * gh; ++c) map[c] = 0xffffffffu;
        const uint32_t* xy = static_cast<const uint32_t*>(q);
        for (uint32_t i = 0; i < n; ++i) map[xy[2u * i + 1u] * gw + xy[2u * i]] = i;
        return TRAY_OK;
    }
    void pull(const void* q, uint32_t n, const uint32_t* map, const uint32_t* samples, uint32_t* active, uint32_t max_ratio, uint32_t max_spp) {
        groups.push_back(101u);
        const int gw = (int)nt::grid_w(width), gh = (int)nt::grid_h(height);
        const uint32_t* xy = static_cast<const uint32_t*>(q);
        const std::vector<uint32_t> before(active, active + n);   // (one Jacobi step: the slowest a launch of the kernel can be)
        for (uint32_t i = 0; i < n; ++i) {
            if (before[i] || samples[i] >= max_spp) continue;
            for (int dy = -1; dy <= 1; ++dy)
                for (int dx = -1; dx <= 1; ++dx) {
                    const int x = (int)xy[2u * i] + dx, y = (int)xy[2u * i + 1u] + dy;
                    if ((!dx && !dy) || x < 0 || y < 0 || x >= gw || y >= gh) continue;
                    const uint32_t u = map[y * gw + x];
                    if (u >= n) continue;
                    if ((uint64_t)samples[u] * (before[u] ? 2u : 1u) > (uint64_t)max_ratio * samples[i]) active[i] = 1u;
                }
        }
    }
    void compact_level(const void* q, const uint32_t* active, const uint32_t* samples, uint32_t n_level, uint32_t n, void* list, uint32_t* list_q, uint32_t* count) {
        groups.push_back(102u);
        uint32_t o = 0u;
        for (uint32_t i = 0; i < n; ++i)
            if (active[i] && samples[i] == n_level) { std::memcpy(static_cast<uint32_t*>(list) + 2u * o, static_cast<const uint32_t*>(q) + 2u * i, 8u); list_q[o++] = i; }
        *count = o;
        lists.push_back({list, list_q});
    }
};

struct Case {
    const char* what;
    uint32_t gw, gh;                          // the frame's tile grid (the frame is 8 gw x 8 gh pixels)
    std::vector<std::pair<uint32_t, uint32_t>> range;   // the call's tiles, in queue order
    std::set<uint32_t> noisy;
    uint32_t min_spp, max_spp, ratio;         // ratio 0: no bound
    std::vector<uint32_t> want;               // n_t per queue entry
    bool filtered = false, with_out = false;
};

struct Outcome { std::vector<uint32_t> n, groups, read_words; uint32_t launches, reads; int bad; };

Outcome run_case(const Case& c, bool through_null_bound = false) {
    const uint32_t n = (uint32_t)c.range.size(), levels = nt::levels_of(c.min_spp, c.max_spp);
    ScriptedOps ops{};
    ops.width = 8u * c.gw; ops.height = 8u * c.gh; ops.noisy = c.noisy; ops.handed.assign(n, 0u);
    for (auto [x, y] : c.range) { ops.queue.push_back(x); ops.queue.push_back(y); }
    const nt::TileLayout tl = nt::tile_layout(n);
    const nt::BoundLayout bl = nt::bound_layout(n, c.gw, c.gh, levels);
    std::vector<unsigned char> tiles(tl.total, 0xA5), bound(bl.total, 0xA5), scratch(c.filtered ? nt::filtered_layout(ops.width, ops.height).total : 0u);
    alignas(16) static float even[4], odd[4], out[4];
    const nt::Target t{ops.queue.data(), n, c.min_spp, c.max_spp, 0.5f, even, odd, tiles.data(), n};
    const nt::Filter f{7u, 3u, 0.45f, scratch.data(), c.with_out ? out : nullptr};
    const nt::Bound b{c.ratio, c.gw, c.gh, bound.data()};
    uint32_t launches = 0u;
    const nt::Refusal no = through_null_bound || c.ratio ? nt::run(ops, t, c.filtered ? &f : nullptr, &launches, c.ratio ? &b : nullptr)
                                                         : nt::run(ops, t, c.filtered ? &f : nullptr, &launches);
    int bad = (int)ops.bad + (no.rc != TRAY_OK);
    const uint32_t* samples = reinterpret_cast<const uint32_t*>(tiles.data() + tl.samples.offset);
    Outcome o{std::vector<uint32_t>(samples, samples + n), ops.groups, ops.read_words, launches, ops.reads, 0};
    for (uint32_t q = 0; q < n; ++q) bad += ops.handed[q] != o.n[q];   // the films are the film of [0, n_t) of every tile
    // launches and reads against the plan's counts, from the rounds and groups the run made
    uint32_t rounds = 0u, groups = 0u, errors = 0u;
    for (uint32_t g : ops.groups) { errors += g == nt_record::kError; groups += g == nt_record::kError; }
    if (c.ratio && levels > 1u) {
        uint32_t pulls = 0u;
        for (uint32_t g : ops.groups) pulls += g == 101u;
        rounds = pulls / (levels - 1u);
        const uint32_t want_launches = nt::bound_call_launches(c.filtered, c.with_out, rounds, groups, levels, 1u);
        const uint32_t want_reads = rounds * nt::kBoundReadsPerRound + (c.filtered ? 1u : 0u);
        if (launches != want_launches || ops.reads != want_reads) { std::printf("  WRONG counts: %u launches (plan %u), %u reads (plan %u)\n", launches, want_launches, ops.reads, want_reads); ++bad; }
    } else {
        rounds = errors;
        if (launches != nt::call_launches(c.filtered, c.with_out, rounds, 1u)) ++bad;
    }
    o.bad = bad;
    return o;
}

int check(const Case& c) {
    const Outcome o = run_case(c);
    int bad = o.bad + (o.n != c.want);
    // neighbours of the range within the ratio
    if (c.ratio)
        for (size_t i = 0; i < c.range.size(); ++i)
            for (size_t j = 0; j < c.range.size(); ++j) {
                const int dx = (int)c.range[i].first - (int)c.range[j].first, dy = (int)c.range[i].second - (int)c.range[j].second;
                if (i != j && dx >= -1 && dx <= 1 && dy >= -1 && dy <= 1) bad += (uint64_t)o.n[i] > (uint64_t)c.ratio * o.n[j];
            }
    std::printf("%-58s n =", c.what);
    for (uint32_t v : o.n) std::printf(" %u", v);
    std::printf(", %u launches, %u reads%s\n", o.launches, o.reads, bad ? " WRONG" : "");
    return bad;
}

}  // namespace

int main() {
    int bad = 0;
    const std::vector<std::pair<uint32_t, uint32_t>> strip{{0u, 0u}, {1u, 0u}, {2u, 0u}, {3u, 0u}, {4u, 0u}};
    // (i) a strip, tile 0 never converges: the least fixed point, so no tile is pulled without need
    bad += check({"(i) strip 5x1, ratio 4", 5u, 1u, strip, {0u}, 2u, 64u, 4u, {64u, 16u, 4u, 2u, 2u}});
    bad += check({"(i) strip 5x1, ratio 2", 5u, 1u, strip, {0u}, 2u, 64u, 2u, {64u, 32u, 16u, 8u, 4u}});
    bad += check({"(i) strip 5x1, no bound", 5u, 1u, strip, {0u}, 2u, 64u, 0u, {64u, 2u, 2u, 2u, 2u}});
    bad += check({"(i) strip 5x1, ratio 4, filtered with output", 5u, 1u, strip, {0u}, 2u, 64u, 4u, {64u, 16u, 4u, 2u, 2u}, true, true});
    bad += check({"(i) strip 5x1, ratio 64 = max / min: nothing to pull", 5u, 1u, strip, {0u}, 2u, 64u, 64u, {64u, 2u, 2u, 2u, 2u}});
    bad += check({"(i) strip 5x1, ratio 4, one level", 5u, 1u, strip, {0u}, 8u, 8u, 4u, {8u, 8u, 8u, 8u, 8u}});
    // (ii) 3 x 3, the centre noisy: the eight neighbours alike, the corners among them (Morton order)
    const std::vector<std::pair<uint32_t, uint32_t>> nine{{0u, 0u}, {1u, 0u}, {0u, 1u}, {1u, 1u}, {2u, 0u}, {2u, 1u}, {0u, 2u}, {1u, 2u}, {2u, 2u}};
    bad += check({"(ii) 3x3, centre noisy, ratio 4", 3u, 3u, nine, {3u}, 2u, 64u, 4u, {16u, 16u, 16u, 64u, 16u, 16u, 16u, 16u, 16u}});
    bad += check({"(ii) 3x3, centre noisy, ratio 2", 3u, 3u, nine, {3u}, 2u, 64u, 2u, {32u, 32u, 32u, 64u, 32u, 32u, 32u, 32u, 32u}});
    // (iii) a range over half of a 4 x 2 grid, the noisy tile at the range's edge: the tiles outside neither pull nor are pulled (they are not in
    // the queue at all), and a tile of the range whose only noisy neighbour lies outside it stays
    const std::vector<std::pair<uint32_t, uint32_t>> half{{0u, 0u}, {1u, 0u}, {0u, 1u}, {1u, 1u}};
    bad += check({"(iii) left half of 4x2, tile (1, 0) noisy, ratio 4", 4u, 2u, half, {1u}, 2u, 64u, 4u, {16u, 64u, 16u, 16u}});
    const std::vector<std::pair<uint32_t, uint32_t>> apart{{0u, 0u}, {3u, 0u}, {3u, 1u}};
    bad += check({"(iii) tiles apart in 4x2, (0, 0) noisy, ratio 2", 4u, 2u, apart, {0u}, 2u, 64u, 2u, {64u, 2u, 2u}});

    // (iv) without a bound: the groups of the unbounded call, as the recording Ops lists them for the same count reads
    {
        const Case c{"", 5u, 1u, strip, {0u, 3u}, 2u, 16u, 0u, {}};
        const Outcome direct = run_case(c), through = run_case(c, true);
        const nt_record::Recorded r = nt_record::record(false, false, 40u, 8u, 5u, 5u, 2u, 16u, 1u, direct.read_words.data(), (uint32_t)direct.read_words.size());
        std::vector<uint32_t> recorded;
        for (const nt_record::Row& row : r.rows) recorded.push_back((uint32_t)row.w[0]);
        const bool same = through.groups == direct.groups && through.groups == recorded && through.launches == r.launches && through.n == direct.n;
        std::printf("(iv) b == nullptr: %zu groups, %u launches%s\n", through.groups.size(), through.launches, same ? "" : " WRONG");
        bad += !same + direct.bad + through.bad;
    }
    // (v) the constexpr by hand for the strip at ratio 4, 6 levels: 6 rounds of 1, 1, 1, 2, 2 and 3 level lists (tile 1 joins after round 2, tile 2
    // after round 4); the map, 3 launches per list, 5 pull steps per round, 1, 2, 3, 4, 5, 5 compactions; one read per round
    {
        const Outcome o = run_case({"", 5u, 1u, strip, {0u}, 2u, 64u, 4u, {}});
        const uint32_t by_hand = 1u + 10u * 3u + 6u * 5u + (1u + 2u + 3u + 4u + 5u + 5u);
        const bool ok = o.launches == by_hand && o.reads == 6u && nt::bound_call_launches(false, false, 6u, 10u, 6u, 1u) == by_hand;
        std::printf("(v) strip at ratio 4: %u launches, %u reads, by hand %u%s\n", o.launches, o.reads, by_hand, ok ? "" : " WRONG");
        bad += !ok;
    }
    // the layout: packed, aligned, 64-bit
    for (uint32_t n : {1u, 24u, 32400u, 400000000u}) {
        const nt::BoundLayout l = nt::bound_layout(n, 240u, 135u, 7u);
        bad += l.lists.offset != 0u || l.lists.bytes != 6ull * n * 8u || l.lists_q.offset != l.lists.bytes || l.lists_q.bytes != 6ull * n * 4u ||
               l.map.offset != l.lists_q.offset + l.lists_q.bytes || l.map.bytes != 240ull * 135u * 4u || l.counts.offset != l.map.offset + l.map.bytes ||
               l.counts.bytes != 32u || l.total != l.counts.offset + 32u || l.map.offset % 4u != 0u;
    }
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
