// TEST INFRASTRUCTURE ONLY: tray_rust_amd/csrc/hip/noise_plan.h's rules, layouts and schedule by number, for tests/test_noise_plan.py and the stub and
// GPU tests that compare a call's launches with the plan's (these are exports of libtrayemu_guide.so: emu_guide.cpp includes this file), and for the
// stand-alone noise_plan_check.cpp. RecordingOps has every launch group of the plan and launches nothing: it notes the group with its arguments, every
// pointer as (buffer, byte offset), and answers the count reads from a script. Needs no kernel header.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../tray_rust_amd/csrc/hip/noise_plan.h"

namespace nt_record {
namespace nt = tr_ntplan;

enum Group : uint32_t { kRender, kBlockList, kHalves, kError, kCompact, kRead, kFinalFilter };
enum Buffer : uint64_t { kNull, kQueue, kEven, kOdd, kTiles, kScratch, kOut, kUnknown };
constexpr uint32_t kRowWords = 12u;   // the group, then its arguments in the order of the Ops member (the floats left out)
// group            arguments
// kRender          list, n, begin, end, film
// kBlockList       queue, active, n, flags, list, count
// kHalves          even, odd, records, radius, patch, blocks, n_blocks, fa, fb
// kError           fe, fo, list, list_q, n, taken, max_spp, err, active, samples
// kCompact         queue, active, n, list, list_q, count
// kRead            counts, n_words
// kFinalFilter     even, odd, radius, patch, out, records
struct Row { uint64_t w[kRowWords]; };

struct RecordingOps {
    uint32_t width, height;
    const nt::Target* t;
    const nt::Filter* f;
    uint32_t per_render;              // launches a render reports
    const uint32_t* script;           // the words the reads answer with, in order; zeros once they are used up
    uint32_t n_script, next = 0u;
    std::vector<Row> rows;

    // a pointer as buffer << 56 | byte offset into it
    uint64_t where(const void* p) const {
        if (!p) return kNull << 56;
        const char* const c = static_cast<const char*>(p);
        auto in = [&](const void* base, uint64_t bytes) { return base && c >= static_cast<const char*>(base) && c < static_cast<const char*>(base) + bytes; };
        auto off = [&](uint64_t buffer, const void* base) { return buffer << 56 | (uint64_t)(c - static_cast<const char*>(base)); };
        if (p == t->queue) return kQueue << 56;
        if (p == t->even) return kEven << 56;
        if (p == t->odd) return kOdd << 56;
        if (f && p == f->out) return kOut << 56;
        if (in(t->tiles, nt::tile_layout(t->n_tiles).total)) return off(kTiles, t->tiles);
        if (f && in(f->scratch, nt::filtered_layout(width, height).total)) return off(kScratch, f->scratch);
        return kUnknown << 56;
    }
    void note(uint32_t group, std::initializer_list<uint64_t> args) {
        Row r{};
        r.w[0] = group;
        uint32_t i = 1u;
        for (uint64_t a : args) r.w[i++] = a;
        rows.push_back(r);
    }
    int render(const void* list, uint32_t n, uint32_t begin, uint32_t end, float* film, uint32_t* launches) {
        note(kRender, {where(list), n, begin, end, where(film)});
        *launches += per_render;
        return TRAY_OK;
    }
    int block_list(const void* queue, const uint32_t* active, uint32_t n, uint32_t* flags, uint32_t* list, uint32_t* count) {
        note(kBlockList, {where(queue), where(active), n, where(flags), where(list), where(count)});
        return TRAY_OK;
    }
    int halves(const float* even, const float* odd, void* records, uint32_t radius, uint32_t patch, float, const uint32_t* blocks, uint32_t n_blocks, float* fa,
               float* fb) {
        note(kHalves, {where(even), where(odd), where(records), radius, patch, where(blocks), n_blocks, where(fa), where(fb)});
        return TRAY_OK;
    }
    void error(const float* fe, const float* fo, const void* list, const uint32_t* list_q, uint32_t n, uint32_t taken, uint32_t max_spp, float, float* err,
               uint32_t* active, uint32_t* samples) {
        note(kError, {where(fe), where(fo), where(list), where(list_q), n, taken, max_spp, where(err), where(active), where(samples)});
    }
    void compact(const void* queue, const uint32_t* active, uint32_t n, void* list, uint32_t* list_q, uint32_t* count) {
        note(kCompact, {where(queue), where(active), n, where(list), where(list_q), where(count)});
    }
    int read(const uint32_t* counts, uint32_t n_words, uint32_t* host) {
        note(kRead, {where(counts), n_words});
        for (uint32_t i = 0; i < n_words; ++i) host[i] = next < n_script ? script[next++] : 0u;
        return TRAY_OK;
    }
    int final_filter(const float* even, const float* odd, uint32_t radius, uint32_t patch, float, float* out, void* records) {
        note(kFinalFilter, {where(even), where(odd), radius, patch, where(out), where(records)});
        return TRAY_OK;
    }
};

struct Recorded { std::vector<Row> rows; int rc; uint32_t launches; };

// The schedule of a call over queue[0, tile_count) of a scene of n_tiles tiles and a width x height film, the reads answered from the script; the
// per-tile buffers and the scratch buffer are vectors of the plan's sizes, so that every pointer the schedule forms lies inside one of them.
inline Recorded record(bool filtered, bool with_out, uint32_t width, uint32_t height, uint32_t n_tiles, uint32_t tile_count, uint32_t min_spp, uint32_t max_spp,
                       uint32_t per_render, const uint32_t* script, uint32_t n_script) {
    alignas(16) static float queue[4], even[4], odd[4], out[4];
    std::vector<char> tiles(nt::tile_layout(n_tiles).total), scratch(filtered ? nt::filtered_layout(width, height).total : 0u);
    const nt::Target t{queue, tile_count, min_spp, max_spp, 0.1f, even, odd, tiles.data(), n_tiles};
    const nt::Filter f{7u, 3u, 0.45f, scratch.data(), with_out ? out : nullptr};
    RecordingOps ops{width, height, &t, filtered ? &f : nullptr, per_render, script, n_script, 0u, {}};
    uint32_t launches = 0u;
    const nt::Refusal no = nt::run(ops, t, filtered ? &f : nullptr, &launches);
    return {ops.rows, no.rc, launches};
}

}  // namespace nt_record

extern "C" {

// kBlockListLaunches, kErrorLaunches, kCompactLaunches, halves_launches(0), halves_launches(1), kFinalFilterLaunches, round_launches(raw), (filtered)
void emu_noise_plan_constants(uint32_t* out) {
    namespace nt = tr_ntplan;
    const uint32_t c[] = {nt::kBlockListLaunches, nt::kErrorLaunches, nt::kCompactLaunches, nt::halves_launches(0u), nt::halves_launches(1u), nt::kFinalFilterLaunches,
                          nt::round_launches(false), nt::round_launches(true)};
    for (uint32_t i = 0; i < sizeof c / sizeof *c; ++i) out[i] = c[i];
}
uint32_t emu_noise_plan_call_launches(int filtered, int with_out, uint32_t rounds, uint32_t per_render) {
    return tr_ntplan::call_launches(filtered != 0, with_out != 0, rounds, per_render);
}
// (offset, bytes) of the six regions in the order of the struct, then the total: 13 words
void emu_noise_plan_tile_layout(uint32_t n_tiles, uint64_t* out) {
    const tr_ntplan::TileLayout l = tr_ntplan::tile_layout(n_tiles);
    const tr_ntplan::Region r[] = {l.list, l.list_q, l.active, l.samples, l.err, l.count};
    for (uint32_t i = 0; i < 6u; ++i) { out[2u * i] = r[i].offset; out[2u * i + 1u] = r[i].bytes; }
    out[12] = l.total;
}
void emu_noise_plan_filtered_layout(uint32_t width, uint32_t height, uint64_t* out) {
    const tr_ntplan::FilteredLayout l = tr_ntplan::filtered_layout(width, height);
    const tr_ntplan::Region r[] = {l.records, l.fa, l.fb, l.flags, l.list, l.counts};
    for (uint32_t i = 0; i < 6u; ++i) { out[2u * i] = r[i].offset; out[2u * i + 1u] = r[i].bytes; }
    out[12] = l.total;
}
uint64_t emu_noise_plan_scratch_bytes(uint32_t width, uint32_t height) { return tr_ntplan::filtered_scratch_bytes(width, height); }
uint32_t emu_noise_plan_frame_blocks(uint32_t width, uint32_t height) { return tr_ntplan::frame_blocks(width, height); }
// a call's rules on plain values (the buffers as addresses, never followed); the message's first `cap` bytes into msg; returns the code
int emu_noise_plan_rules(int filtered, int scene, uint32_t sampler_kind, int broken, uint32_t width, uint32_t height, uint32_t min_spp, uint32_t max_spp,
                         float threshold, uintptr_t even, uintptr_t odd, uint32_t radius, uint32_t patch, float k, uintptr_t out, uintptr_t scratch,
                         uintptr_t tile_samples, uintptr_t tile_error, char* msg, uint32_t cap) {
    namespace nt = tr_ntplan;
    auto p = [](uintptr_t a) { return reinterpret_cast<const void*>(a); };
    const nt::Scene s{scene != 0, sampler_kind, broken != 0, width, height};
    const nt::Refusal no = filtered ? nt::filtered_rules("filtered", s, min_spp, max_spp, threshold, p(even), p(odd), radius, patch, k, p(out), p(scratch),
                                                         p(tile_samples), p(tile_error))
                                    : nt::target_rules("raw", s, min_spp, max_spp, threshold, p(even), p(odd), p(tile_samples), p(tile_error));
    if (msg && cap) { std::strncpy(msg, no.msg.c_str(), cap - 1u); msg[cap - 1u] = 0; }
    return no.rc;
}
// the schedule's launch groups, kRowWords words each, the first `cap` of them; *rc: what the schedule returned, *launches: what it counted; returns
// the number of groups
uint32_t emu_noise_plan_record(int filtered, int with_out, uint32_t width, uint32_t height, uint32_t n_tiles, uint32_t tile_count, uint32_t min_spp,
                               uint32_t max_spp, uint32_t per_render, const uint32_t* script, uint32_t n_script, uint64_t* rows, uint32_t cap, int* rc,
                               uint32_t* launches) {
    const nt_record::Recorded r = nt_record::record(filtered != 0, with_out != 0, width, height, n_tiles, tile_count, min_spp, max_spp, per_render, script, n_script);
    for (uint32_t i = 0; i < r.rows.size() && i < cap; ++i) std::memcpy(rows + (size_t)nt_record::kRowWords * i, r.rows[i].w, sizeof r.rows[i].w);
    *rc = r.rc;
    *launches = r.launches;
    return (uint32_t)r.rows.size();
}

}  // extern "C"
