// TEST INFRASTRUCTURE ONLY: tray_rust_amd/csrc/hip/wavefront_plan.h's rules, layout and round by number, for tests/test_wavefront_plan.py (these are
// exports of libtrayemu.so: emu_kernels.cpp includes this file) and for the stand-alone wavefront_plan_check.cpp. RecordingOps has every launch group
// of the plan and launches nothing: it notes the group with its stage or material kind, the queue it reads, the queue it fills and the fused flag.
// Include after kernels.hip and wavefront_plan.h.
#pragma once
#include <cstdint>
#include <vector>

namespace wf_record {
namespace wp = tr_wfplan;

enum Group : uint32_t { kAdvance, kRegen, kBin, kTrace, kClearQctl, kSort, kShadeKind, kBegin, kQueryKind, kQuery };
constexpr uint32_t kNone = 255u;   // no stage / kind, no queue
struct Launch { uint32_t group, stage, from, to, fused; };   // stage: S of bin / trace, K of the kind launches; trace's `to`: the fallback records' buffer

struct RecordingOps {
    std::vector<Launch> launches;
    void note(uint32_t group, uint32_t stage, uint32_t from, uint32_t to, uint32_t fused = 0u) { launches.push_back({group, stage, from, to, fused}); }
    static uint32_t qc(bool stage_c) { return stage_c ? (uint32_t)wp::QC : kNone; }
    template <int ANIM> void advance() { note(kAdvance, kNone, kNone, wp::QA); }
    template <int ANIM> void regen() { note(kRegen, kNone, wp::QR, wp::QA); }
    template <int S> void bin(wp::Queue from, wp::Queue to) { note(kBin, S, from, to); }
    template <int S, int ANIM> void trace(wp::Queue from, wp::Queue fallback, uint32_t fused) { note(kTrace, S, from, fallback, fused); }
    int clear_qctl() { note(kClearQctl, kNone, kNone, kNone); return 0; }
    int clear_bin_ctl() { return 0; }
    void sort() { note(kSort, kNone, kNone, kNone); }
    template <int ANIM, int K> void shade_kind() { note(kShadeKind, K, kNone, wp::QB); }
    template <int ANIM> void begin() { note(kBegin, kNone, kNone, wp::QB); }
    template <int ANIM, int K> void query_kind(bool stage_c) { note(kQueryKind, K, kNone, qc(stage_c)); }
    template <int ANIM> void query(bool stage_c) { note(kQuery, kNone, kNone, qc(stage_c)); }
};

inline std::vector<Launch> record_round(bool anim, const wp::RoundCfg& c) {
    RecordingOps ops;
    if (anim) wp::round<1>(ops, c); else wp::round<0>(ops, c);
    return ops.launches;
}

}  // namespace wf_record

extern "C" {

// WF_SEGS, TR_BLOCK, WF_RAY_WORDS, WF_QCTL_WORDS, WF_BINS, WF_MAT_KINDS, WF_PIPES_MAX, WF_POLL, WF_FOLD_C
void emu_wf_plan_constants(uint32_t* out) {
    const uint32_t c[] = {WF_SEGS, TR_BLOCK, WF_RAY_WORDS, WF_QCTL_WORDS, WF_BINS, WF_MAT_KINDS, WF_PIPES_MAX, WF_POLL, WF_FOLD_C};
    for (uint32_t i = 0; i < sizeof c / sizeof *c; ++i) out[i] = c[i];
}
// the Layout's 13 fields in the order of the struct
void emu_wf_plan_layout(uint32_t pool_chunks, uint32_t full_depth, uint32_t lds_depth, uint32_t n_blocks_trace, uint64_t* out) {
    const tr_wfplan::Layout l = tr_wfplan::layout(pool_chunks, full_depth, lds_depth, n_blocks_trace);
    const uint64_t f[] = {l.q_total, l.q_word[0], l.q_word[1], l.q_word[2], l.q_word[3], l.qctl_word, l.bin_ctl_words, l.kind_entries, l.ovf_entries,
                          l.queue_bytes, l.bin_ctl_bytes, l.kind_bytes, l.ovf_bytes};
    for (uint32_t i = 0; i < sizeof f / sizeof *f; ++i) out[i] = f[i];
}
// view k of n_views over n_chunks chunks of that layout: first_chunk, n_chunks, seg_cap, q_off, qctl_word, bin_ctl_word, ovf_entry
void emu_wf_plan_view(uint32_t pool_chunks, uint32_t full_depth, uint32_t lds_depth, uint32_t n_blocks_trace, uint32_t k, uint32_t n_views, uint32_t n_chunks,
                      uint64_t* out) {
    const tr_wfplan::View v = tr_wfplan::view(tr_wfplan::layout(pool_chunks, full_depth, lds_depth, n_blocks_trace), k, n_views, n_chunks);
    const uint64_t f[] = {v.first_chunk, v.n_chunks, v.seg_cap, v.q_off, v.qctl_word, v.bin_ctl_word, v.ovf_entry};
    for (uint32_t i = 0; i < sizeof f / sizeof *f; ++i) out[i] = f[i];
}
uint32_t emu_wf_plan_view_count(uint32_t n_chunks, uint32_t req_views) { return tr_wfplan::view_count(n_chunks, req_views); }
uint64_t emu_wf_plan_max_rounds(uint32_t n_items, uint32_t n_chunks, uint32_t n, uint32_t slice_shift, uint32_t max_depth) {
    return tr_wfplan::max_rounds(n_items, n_chunks, n, slice_shift, max_depth);
}
uint32_t emu_wf_plan_nominal_launches(uint32_t bin_stages) { return tr_wfplan::nominal_launches(bin_stages); }
// one round's launch groups, five words each (wf_record::Launch), the first `cap` of them; returns their number
uint32_t emu_wf_plan_round(int anim, int sorted, int fused, uint32_t bin_stages, int bin_ctl, uint32_t kinds_present, uint32_t* out, uint32_t cap) {
    const std::vector<wf_record::Launch> l = wf_record::record_round(anim != 0, tr_wfplan::RoundCfg{sorted != 0, fused != 0, bin_stages, bin_ctl != 0, kinds_present});
    for (uint32_t i = 0; i < l.size() && i < cap; ++i) {
        const uint32_t w[5] = {l[i].group, l[i].stage, l[i].from, l[i].to, l[i].fused};
        for (uint32_t j = 0; j < 5u; ++j) out[5u * i + j] = w[j];
    }
    return (uint32_t)l.size();
}

}  // extern "C"
