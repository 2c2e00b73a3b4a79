// What the two noise-target calls (include/trayhip.h: tray_render_noise_target_device, tray_render_noise_target_filtered_device) decide on the host:
// which arguments they refuse, where the regions of a scene's per-tile buffers and of the filtered rule's scratch buffer lie, and which launches the
// rounds make in which order, with the one host read that ends a round. Host-only functions of the calls' plain arguments -- no HIP call, no
// stream, no kernel header, as denoise_plan.h: device_api.hip runs the schedule with an Ops that forwards to launch_tiles and the add-on libraries'
// launch functions (noise.h, guide.h, denoise.h), the host emulation (tests/emu/emu_guide.cpp) with an Ops that launches the kernels as fibers.
#pragma once

#include "denoise_plan.h"

namespace tr_ntplan {

using tr_dnplan::Refusal;
using tr_dnplan::Region;
using tr_dnplan::at;
using tr_dnplan::film_at;

// ---- rules: {TRAY_OK, ""} or the refusal's return code and message, in the order the calls have always checked them. What depends on the scene
// arrives as plain values (no scene: the other three are not read); `who` names the call in the message.

struct Scene { bool given; uint32_t sampler_kind; bool broken; uint32_t width, height; };

inline Refusal target_rules(const std::string& who, const Scene& s, uint32_t min_spp, uint32_t max_spp, float threshold, const void* even, const void* odd,
                            const void* tile_samples, const void* tile_error) {
    if (!s.given || !even || !odd || !tile_samples || !tile_error) return {TRAY_E_INVALID, who + ": null argument"};
    auto pow2 = [](uint32_t v) { return v != 0u && (v & (v - 1u)) == 0u; };
    if (!pow2(min_spp) || !pow2(max_spp) || min_spp < 2u || max_spp < min_spp)
        return {TRAY_E_INVALID, who + ": min_spp and max_spp must be powers of two with 2 <= min_spp <= max_spp"};
    if (!(threshold >= 0.0f)) return {TRAY_E_INVALID, who + ": threshold must be >= 0 (and not NaN)"};
    if (even == odd) return {TRAY_E_INVALID, who + ": the even and odd films must be different buffers"};
    if (s.sampler_kind != TRAY_SAMPLER_LOW_DISCREPANCY) return {TRAY_E_UNSUPPORTED, who + ": sample ranges exist for the LowDiscrepancy sampler only"};
    if (s.broken) return {TRAY_E_INVALID, "this device scene is unusable: a tray_scene_update_frame on it failed"};
    return {TRAY_OK, ""};
}
// the filtered call's: those, then its scratch buffer, the filter's own rules, and the three or four buffers all different and aligned
inline Refusal filtered_rules(const std::string& who, const Scene& s, uint32_t min_spp, uint32_t max_spp, float threshold, const void* even, const void* odd,
                              uint32_t radius, uint32_t patch, float k, const void* out, const void* scratch, const void* tile_samples,
                              const void* tile_error) {
    if (Refusal r = target_rules(who, s, min_spp, max_spp, threshold, even, odd, tile_samples, tile_error); r.rc != TRAY_OK) return r;
    if (!scratch) return {TRAY_E_INVALID, who + ": null argument"};
    if (Refusal r = tr_dnplan::filter_args(who, s.width, s.height, radius, patch, k); r.rc != TRAY_OK) return r;
    const void* const bufs[4] = {even, odd, scratch, out};
    if (!tr_dnplan::distinct_aligned(bufs, out ? 4u : 3u))
        return {TRAY_E_INVALID, who + ": the films, the output and the scratch buffer must be different buffers, 16-byte aligned"};
    return {TRAY_OK, ""};
}

// ---- layouts: byte offsets from the buffer's base, packed in the order of the struct's members, and their total; 64-bit arithmetic throughout

// a scene's per-tile buffers, n_tiles entries each: the compacted list (x, y) and its queue indices, then per queue entry the flag, the samples taken
// and the error; one count word behind them
struct TileLayout { Region list, list_q, active, samples, err, count; uint64_t total; };
inline TileLayout tile_layout(uint32_t n_tiles) {
    uint64_t end = 0u;
    auto take = [&](uint64_t bytes) { const Region r{end, bytes}; end += bytes; return r; };
    const uint64_t n = n_tiles;
    return {take(n * 8u), take(n * 4u), take(n * 4u), take(n * 4u), take(n * 4u), take(4u), end};
}

// the 32 x 16 blocks of a frame (k_dn_filter's tiles; device_api.hip ties the two constants to the guide library's)
inline uint32_t blocks_x(uint32_t width) { return (width + TRAY_DENOISE_BLOCK_W - 1u) / TRAY_DENOISE_BLOCK_W; }
inline uint32_t blocks_y(uint32_t height) { return (height + TRAY_DENOISE_BLOCK_H - 1u) / TRAY_DENOISE_BLOCK_H; }
inline uint32_t frame_blocks(uint32_t width, uint32_t height) { return blocks_x(width) * blocks_y(height); }

// the filtered rule's private scratch: the filter's records (plain_layout), the filtered halves fa and fb, one flag and one list word per block, and
// the counts: active tiles, listed blocks, two words of padding
struct FilteredLayout { Region records, fa, fb, flags, list, counts; uint64_t total; };
inline FilteredLayout filtered_layout(uint32_t width, uint32_t height) {
    tr_dnplan::Packer s(width, height);
    const Region records = s.take((uint32_t)tr_dnplan::plain_layout(1u, 1u).total), fa = s.take(tr_dnplan::kFilmBytes), fb = s.take(tr_dnplan::kFilmBytes);
    const uint64_t nb = (uint64_t)blocks_x(width) * blocks_y(height);
    const Region flags{s.end, nb * 4u}, list{flags.offset + flags.bytes, nb * 4u}, counts{list.offset + list.bytes, 16u};
    return {records, fa, fb, flags, list, counts, counts.offset + counts.bytes};
}
// tray_noise_target_filtered_scratch_bytes: 0 for an empty frame
inline uint64_t filtered_scratch_bytes(uint32_t width, uint32_t height) { return width == 0u || height == 0u ? 0u : filtered_layout(width, height).total; }

// ---- launch counts of the groups below (a render's is the Ops's to say: the wavefront schedule's depends on its rounds)
constexpr uint32_t kBlockListLaunches = 2u;                                  // k_guide_mark, k_guide_compact (the memset of the flags is no launch)
constexpr uint32_t kErrorLaunches = 1u, kCompactLaunches = 1u;
constexpr uint32_t halves_launches(uint32_t n_blocks) { return tr_dnplan::kPrepareLaunches + (n_blocks ? 1u : 0u); }   // (an empty list: the halves launch nothing)
constexpr uint32_t kFinalFilterLaunches = tr_dnplan::kDenoiseLaunches;
// a round's launches besides its two renders, over a non-empty block list, and a whole call's of `rounds` rounds with r launches per render
constexpr uint32_t round_launches(bool filtered) { return kErrorLaunches + kCompactLaunches + (filtered ? halves_launches(1u) + kBlockListLaunches : 0u); }
constexpr uint32_t call_launches(bool filtered, bool out, uint32_t rounds, uint32_t r) {
    return (filtered ? kBlockListLaunches : 0u) + rounds * (2u * r + round_launches(filtered)) + (filtered && out ? kFinalFilterLaunches : 0u);
}
static_assert(call_launches(false, false, 1u, 1u) == 4u && call_launches(true, false, 1u, 1u) == 11u && call_launches(true, true, 3u, 1u) == 32u,
              "4 launches per round of the raw rule; 2 + 9 per round (+ 3) of the filtered one");

// ---- the neighbour bound (include/trayhip.h: tray_scene_set_noise_ratio)

constexpr uint32_t kMaxLevels = 16u;   // min_spp 2 ... max_spp 65536: bound_rules refuses a bound over more levels
// the levels of a call: a tile's n_t is min_spp 2^l, l in [0, levels)
constexpr uint32_t levels_of(uint32_t min_spp, uint32_t max_spp) {
    uint32_t l = 1u;
    for (uint64_t n = min_spp; n < max_spp; n *= 2u) ++l;
    return l;
}
// the tiles of the grid the 8 x 8 tiles of a width x height frame form
inline uint32_t grid_w(uint32_t width) { return (width + 7u) / 8u; }
inline uint32_t grid_h(uint32_t height) { return (height + 7u) / 8u; }

// the bound's own per-tile buffers, beside tile_layout's: per level that can render (all but the last) a tile list (x, y) and its queue indices, n_tiles
// entries each; the map from a tile's cell of the grid to its queue index; the count words: [0] the filtered rule's listed blocks, [1 + l] level l's tiles
struct BoundLayout { Region lists, lists_q, map, counts; uint64_t total; };
inline BoundLayout bound_layout(uint32_t n_tiles, uint32_t gw, uint32_t gh, uint32_t levels) {
    uint64_t end = 0u;
    auto take = [&](uint64_t bytes) { const Region r{end, bytes}; end += bytes; return r; };
    const uint64_t n = n_tiles, rendering = levels > 1u ? levels - 1u : 1u;
    return {take(rendering * n * 8u), take(rendering * n * 4u), take((uint64_t)gw * gh * 4u), take(((uint64_t)levels + 1u) * 4u), end};
}

// what a call under tray_scene_set_noise_ratio refuses beyond its own rules (max_ratio itself is the setter's to judge)
inline Refusal bound_rules(const std::string& who, uint32_t max_ratio, uint32_t min_spp, uint32_t max_spp) {
    if (max_ratio != 0u && levels_of(min_spp, max_spp) > kMaxLevels)
        return {TRAY_E_INVALID, who + ": under tray_scene_set_noise_ratio max_spp is at most 32768 min_spp (16 values of n_t)"};
    return {TRAY_OK, ""};
}

constexpr uint32_t kGridLaunches = 1u, kPullLaunches = 1u, kCompactLevelLaunches = 1u;   // (the memset of the map is no launch)
// the level lists round `round` (from 0) compacts: those of the levels a tile can stand at by then, the last level left out (it never renders)
constexpr uint32_t round_lists(uint32_t round, uint32_t levels) { return levels < 2u ? 0u : (round + 1u < levels - 1u ? round + 1u : levels - 1u); }
// a bounded call's launches: `rounds` rounds that rendered `groups` non-empty level lists between them (one in round 0), r launches per render. Every
// group is its two renders, the filtered halves and the error launch; every round ends with levels - 1 pull steps, its level lists and, filtered, the
// next block list; the map is made once. (levels >= 2: a call over one level runs the unbounded schedule)
constexpr uint32_t bound_call_launches(bool filtered, bool out, uint32_t rounds, uint32_t groups, uint32_t levels, uint32_t r) {
    uint32_t n = (filtered ? kBlockListLaunches : 0u) + kGridLaunches + groups * (2u * r + kErrorLaunches + (filtered ? halves_launches(1u) : 0u));
    for (uint32_t i = 0u; i < rounds; ++i)
        n += (levels - 1u) * kPullLaunches + round_lists(i, levels) * kCompactLevelLaunches + (filtered ? kBlockListLaunches : 0u);
    return n + (filtered && out ? kFinalFilterLaunches : 0u);
}
constexpr uint32_t kBoundReadsPerRound = 1u;   // the round's one synchronisation: one count per level list (and the block count) in one copy
static_assert(levels_of(16u, 1024u) == 7u && levels_of(2u, 2u) == 1u && round_lists(0u, 7u) == 1u && round_lists(9u, 7u) == 6u, "7 levels from 16 to 1024");
static_assert(bound_call_launches(false, false, 1u, 1u, 2u, 1u) == 6u && bound_call_launches(true, true, 2u, 3u, 3u, 1u) == 2u + 1u + 3u * 6u + 2u * 4u + 3u + 3u,
              "grid, then 2 renders + error per group, then pulls and lists per round");

// ---- the schedule

// what both calls take: queue[0, tile_count) of (x, y) tiles, the two films, and the scene's per-tile buffers (tile_layout(n_tiles), tile_count <= n_tiles)
struct Target {
    const void* queue;
    uint32_t tile_count, min_spp, max_spp;
    float threshold;
    float* even, * odd;
    void* tiles;
    uint32_t n_tiles;
};
// what the filtered rule adds: the filter's arguments, its scratch buffer (filtered_layout) and the output of the final filter, or null
struct Filter { uint32_t radius, patch; float k; void* scratch; float* out; };
// what the neighbour bound adds: max_ratio (a power of two >= 2) and its buffers (bound_layout(t.n_tiles, grid_w, grid_h, levels_of(min_spp, max_spp)))
struct Bound { uint32_t max_ratio, grid_w, grid_h; void* mem; };

// Ops has width and height and one member per launch group; those that can fail return TRAY_OK or a code, which run() hands on with an empty message:
//   int render(list, n, begin, end, film, &launches)      samples [begin, end) of the n tiles of `list` into film; adds its launches
//   int block_list(queue, active, n, flags, list, count)  the blocks that hold a tile of queue[0, n) whose flag is set (active null: every tile), in
//                                                         row-major order into list, their number into *count: memset of the flags, mark, compact
//   int halves(even, odd, records, radius, patch, k, blocks, n_blocks, fa, fb)       prepare, then the halves over the block list: halves_launches(n_blocks)
//   void error(fe, fo, list, list_q, n, taken, max_spp, threshold, err, active, samples)
//   void compact(queue, active, n, list, list_q, count)
//   int read(counts, n_words, host)                       the device words counts[0, n_words) into host[]: the round's only synchronisation
//   int final_filter(even, odd, radius, patch, k, out, records)
// and for a bounded call (b given), over the grid of grid_w(width) x grid_h(height) tiles:
//   int grid(queue, n, map)                               map[cell] = the queue index of the tile there, 0xffffffff where queue[0, n) has none
//   void pull(queue, n, map, samples, active, max_ratio, max_spp)      one step of rule (b): sets flags, clears none
//   void compact_level(queue, active, samples, n_level, n, list, list_q, count)   compact() over the flagged tiles with samples == n_level
//
// The rounds over queue[0, tile_count): round r renders [lo, hi) -- [0, min_spp), then [min_spp 2^(r-1), min_spp 2^r) -- of the active tiles, [lo, mid)
// into even and [mid, hi) into odd; then the error kernel writes every active tile's error, samples and flag, the compaction the next list in queue
// order, and the host reads its length once. Round 0's list is the queue itself (queue index = list index: no list_q), later rounds' the compacted
// one. With f (the filtered rule) the error is taken from the filtered halves of the films as they stand, computed over the blocks that hold an active
// tile; the round also makes the next block list and the host reads both lengths in its one copy (round 0's blocks, those that hold a tile of the
// range, are a read of their own before it). The rounds end when no tile is active or at max_spp (no flag is set there: the list is empty then too);
// then the final filter of the films into f->out, if given. *launches counts every launch made, also when a round refuses.
//
// With a bound b over two levels or more (include/trayhip.h, "Neighbour bound") every tile carries its own n_t, so a round renders one list per level:
// for each non-empty level, lowest first, exactly the round above without its compaction -- the two renders of [n, 1.5 n) and [1.5 n, 2 n) of the level's
// list, the filtered halves, the error launch with taken = 2 n --; then, once, levels - 1 pull steps over the queue (the longest chain of pulls, so
// the flags are rule (b)'s least fixed point without a host read), one ordered compaction per level a tile can stand at (round_lists), the filtered
// rule's next block list, and the round's one read: a count per level list. The rounds end when every list is empty. Without b, or over one
// level, the calls on Ops are those above, in that order.
template <class Ops>
inline Refusal run_bounded(Ops& ops, const Target& t, const Filter* f, uint32_t* launches, const Bound& b);

// (run's trailing `const Bound* b = nullptr`, as two overloads: an Ops that is only ever run without a bound needs none of the bound's members)
template <class Ops>
inline Refusal run(Ops& ops, const Target& t, const Filter* f, uint32_t* launches);
template <class Ops>
inline Refusal run(Ops& ops, const Target& t, const Filter* f, uint32_t* launches, const Bound* b) {
    return b && t.min_spp < t.max_spp ? run_bounded(ops, t, f, launches, *b) : run(ops, t, f, launches);
}

template <class Ops>
inline Refusal run(Ops& ops, const Target& t, const Filter* f, uint32_t* launches) {
    const TileLayout tl = tile_layout(t.n_tiles);
    void* const c_list = at(t.tiles, tl.list);
    uint32_t* const c_list_q = static_cast<uint32_t*>(at(t.tiles, tl.list_q)), * const active = static_cast<uint32_t*>(at(t.tiles, tl.active));
    uint32_t* const samples = static_cast<uint32_t*>(at(t.tiles, tl.samples));
    float* const err = film_at(t.tiles, tl.err);
    FilteredLayout fl{};
    float* fa = nullptr, * fb = nullptr;
    uint32_t* flags = nullptr, * blocks = nullptr;
    uint32_t* counts = static_cast<uint32_t*>(at(t.tiles, tl.count));   // [0]: active tiles; the filtered rule's own: [1]: listed blocks
    if (f) {
        fl = filtered_layout(ops.width, ops.height);
        fa = film_at(f->scratch, fl.fa); fb = film_at(f->scratch, fl.fb);
        flags = static_cast<uint32_t*>(at(f->scratch, fl.flags)); blocks = static_cast<uint32_t*>(at(f->scratch, fl.list));
        counts = static_cast<uint32_t*>(at(f->scratch, fl.counts));
    }
    const void* list = t.queue;
    const uint32_t* list_q = nullptr;
    uint32_t host[2] = {0u, 0u};
    uint32_t n_active = t.tile_count, n_blocks = 0u;
    if (f) {
        if (const int rc = ops.block_list(t.queue, nullptr, t.tile_count, flags, blocks, counts + 1); rc != TRAY_OK) return {rc, ""};
        *launches += kBlockListLaunches;
        if (const int rc = ops.read(counts + 1, 1u, host + 1); rc != TRAY_OK) return {rc, ""};
        n_blocks = host[1];
    }
    for (uint32_t lo = 0u, hi = t.min_spp;; lo = hi, hi *= 2u) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (const int rc = ops.render(list, n_active, lo, mid, t.even, launches); rc != TRAY_OK) return {rc, ""};
        if (const int rc = ops.render(list, n_active, mid, hi, t.odd, launches); rc != TRAY_OK) return {rc, ""};
        const float* fe = t.even, * fo = t.odd;   // the two films the error is taken from
        if (f) {
            if (n_blocks > frame_blocks(ops.width, ops.height))
                return {TRAY_E_DEVICE, "tray_render_noise_target_filtered_device: the block list is longer than the frame has blocks"};
            if (const int rc = ops.halves(t.even, t.odd, at(f->scratch, fl.records), f->radius, f->patch, f->k, blocks, n_blocks, fa, fb); rc != TRAY_OK) return {rc, ""};
            *launches += halves_launches(n_blocks);
            fe = fa; fo = fb;
        }
        ops.error(fe, fo, list, list_q, n_active, hi, t.max_spp, t.threshold, err, active, samples);
        ops.compact(t.queue, active, t.tile_count, c_list, c_list_q, counts);
        *launches += kErrorLaunches + kCompactLaunches;
        if (f) {
            if (const int rc = ops.block_list(t.queue, active, t.tile_count, flags, blocks, counts + 1); rc != TRAY_OK) return {rc, ""};
            *launches += kBlockListLaunches;
        }
        if (const int rc = ops.read(counts, f ? 2u : 1u, host); rc != TRAY_OK) return {rc, ""};
        n_active = host[0];
        n_blocks = host[1];
        if (n_active > t.tile_count) return {TRAY_E_DEVICE, "tray_render_noise_target_device: the compacted tile list is longer than the queue"};
        if (n_active == 0u || hi >= t.max_spp) break;
        list = c_list; list_q = c_list_q;
    }
    if (f && f->out) {
        if (const int rc = ops.final_filter(t.even, t.odd, f->radius, f->patch, f->k, f->out, at(f->scratch, fl.records)); rc != TRAY_OK) return {rc, ""};
        *launches += kFinalFilterLaunches;
    }
    return {TRAY_OK, ""};
}

template <class Ops>
inline Refusal run_bounded(Ops& ops, const Target& t, const Filter* f, uint32_t* launches, const Bound& b) {
    const uint32_t levels = levels_of(t.min_spp, t.max_spp);
    if (const Refusal no = bound_rules("tray_render_noise_target_device", b.max_ratio, t.min_spp, t.max_spp); no.rc != TRAY_OK) return no;
    const TileLayout tl = tile_layout(t.n_tiles);
    const BoundLayout bl = bound_layout(t.n_tiles, b.grid_w, b.grid_h, levels);
    uint32_t* const active = static_cast<uint32_t*>(at(t.tiles, tl.active)), * const samples = static_cast<uint32_t*>(at(t.tiles, tl.samples));
    float* const err = film_at(t.tiles, tl.err);
    uint32_t* const map = static_cast<uint32_t*>(at(b.mem, bl.map)), * const counts = static_cast<uint32_t*>(at(b.mem, bl.counts));
    // level l's list and its queue indices
    auto list_of = [&](uint32_t l) { return at(b.mem, Region{bl.lists.offset + (uint64_t)l * t.n_tiles * 8u, 8u}); };
    auto list_q_of = [&](uint32_t l) { return static_cast<uint32_t*>(at(b.mem, Region{bl.lists_q.offset + (uint64_t)l * t.n_tiles * 4u, 4u})); };
    FilteredLayout fl{};
    float* fa = nullptr, * fb = nullptr;
    uint32_t* flags = nullptr, * blocks = nullptr;
    uint32_t host[kMaxLevels + 1u] = {};
    uint32_t n_blocks = 0u;
    if (f) {
        fl = filtered_layout(ops.width, ops.height);
        fa = film_at(f->scratch, fl.fa); fb = film_at(f->scratch, fl.fb);
        flags = static_cast<uint32_t*>(at(f->scratch, fl.flags)); blocks = static_cast<uint32_t*>(at(f->scratch, fl.list));
        if (const int rc = ops.block_list(t.queue, nullptr, t.tile_count, flags, blocks, counts); rc != TRAY_OK) return {rc, ""};
        *launches += kBlockListLaunches;
        if (const int rc = ops.read(counts, 1u, host); rc != TRAY_OK) return {rc, ""};
        n_blocks = host[0];
    }
    if (const int rc = ops.grid(t.queue, t.tile_count, map); rc != TRAY_OK) return {rc, ""};
    *launches += kGridLaunches;
    // one level's list of a round: the round of run() without its compaction
    auto group = [&](const void* list, const uint32_t* list_q, uint32_t n, uint32_t lo, uint32_t hi) -> Refusal {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (const int rc = ops.render(list, n, lo, mid, t.even, launches); rc != TRAY_OK) return {rc, ""};
        if (const int rc = ops.render(list, n, mid, hi, t.odd, launches); rc != TRAY_OK) return {rc, ""};
        const float* fe = t.even, * fo = t.odd;
        if (f) {
            if (n_blocks > frame_blocks(ops.width, ops.height))
                return {TRAY_E_DEVICE, "tray_render_noise_target_filtered_device: the block list is longer than the frame has blocks"};
            if (const int rc = ops.halves(t.even, t.odd, at(f->scratch, fl.records), f->radius, f->patch, f->k, blocks, n_blocks, fa, fb); rc != TRAY_OK) return {rc, ""};
            *launches += halves_launches(n_blocks);
            fe = fa; fo = fb;
        }
        ops.error(fe, fo, list, list_q, n, hi, t.max_spp, t.threshold, err, active, samples);
        *launches += kErrorLaunches;
        return {TRAY_OK, ""};
    };
    uint32_t n_level[kMaxLevels] = {};   // the lengths of the level lists the round renders
    for (uint32_t round = 0u;; ++round) {
        if (round == 0u) {
            if (const Refusal no = group(t.queue, nullptr, t.tile_count, 0u, t.min_spp); no.rc != TRAY_OK) return no;
        } else {
            for (uint32_t l = 0u; l + 1u < levels; ++l) {
                if (n_level[l] == 0u) continue;
                const uint32_t n = t.min_spp << l;
                if (const Refusal no = group(list_of(l), list_q_of(l), n_level[l], n, 2u * n); no.rc != TRAY_OK) return no;
            }
        }
        for (uint32_t i = 0u; i + 1u < levels; ++i) ops.pull(t.queue, t.tile_count, map, samples, active, b.max_ratio, t.max_spp);
        *launches += (levels - 1u) * kPullLaunches;
        const uint32_t lists = round_lists(round, levels);
        for (uint32_t l = 0u; l < lists; ++l) ops.compact_level(t.queue, active, samples, t.min_spp << l, t.tile_count, list_of(l), list_q_of(l), counts + 1u + l);
        *launches += lists * kCompactLevelLaunches;
        if (f) {
            if (const int rc = ops.block_list(t.queue, active, t.tile_count, flags, blocks, counts); rc != TRAY_OK) return {rc, ""};
            *launches += kBlockListLaunches;
        }
        if (const int rc = f ? ops.read(counts, 1u + lists, host) : ops.read(counts + 1u, lists, host + 1u); rc != TRAY_OK) return {rc, ""};
        n_blocks = host[0];
        uint64_t n_active = 0u;
        for (uint32_t l = 0u; l + 1u < levels; ++l) { n_level[l] = l < lists ? host[1u + l] : 0u; n_active += n_level[l]; }
        if (n_active > t.tile_count) return {TRAY_E_DEVICE, "tray_render_noise_target_device: the compacted tile lists are longer than the queue"};
        if (n_active == 0u) break;
    }
    if (f && f->out) {
        if (const int rc = ops.final_filter(t.even, t.odd, f->radius, f->patch, f->k, f->out, at(f->scratch, fl.records)); rc != TRAY_OK) return {rc, ""};
        *launches += kFinalFilterLaunches;
    }
    return {TRAY_OK, ""};
}

}  // namespace tr_ntplan
