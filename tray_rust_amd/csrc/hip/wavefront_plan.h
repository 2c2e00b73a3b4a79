// The wavefront schedule on the host (wavefront.h's stage kernels): the rules of a launch, the shape of the queue buffers and their cut into views,
// the order of a round's launches and the round / poll loop. Host-only -- no kernel, no HIP call, no device scene: device_api.hip runs the schedule with
// an Ops that launches on a view's stream, the host emulation (tests/emu) compiles this header under g++ and runs the same schedule with an Ops that
// launches the kernels as fibers, so it tests the library's schedule and keeps no copy of it. The measurements next to a rule are why its numbers are
// what they are; environment overrides that belong to a rule are read here. Include after kernels.hip (WF_SEGS, wf_seg_cap, WF_RAY_WORDS,
// WF_QCTL_WORDS, WF_BINS, WF_MAT_KINDS, WF_FOLD_C, TR_BLOCK).
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cstdlib>
#include <type_traits>

#ifndef WF_PIPES_MAX
#define WF_PIPES_MAX 4   // views of the wavefront schedule the buffers are sized for
#endif
#define WF_POLL 16       // the library reads the "tiles done" word every WF_POLL rounds; kernels of finished chunks exit at once

namespace tr_wfplan {

// ---- rules

// fused shading (wavefront.h: k_wf_sort + k_wf_shade_kind) is wanted; TRAYHIP_WF_FUSED=0|1 overrides
inline bool fused_wanted() {
    if (const char* e = getenv("TRAYHIP_WF_FUSED")) return atoi(e) != 0;
    return WF_FUSED_DEFAULT != 0;
}
// stages whose rays are binned before the traversal: bit 0 = A, bit 1 = B; TRAYHIP_WF_BIN overrides
inline uint32_t bin_stages_wanted() {
    if (const char* e = getenv("TRAYHIP_WF_BIN")) return (uint32_t)std::max(0, atoi(e)) & 3u;
    return WF_BIN_DEFAULT;
}
// the views: equal shares of the chunks in use. Measured on the C5 stand-in at full detail (1 / 2 / 3 / 4 views): see DESIGN.md section 4
// (with rounds of 24 M slots and more one view is ahead: C5 stand-in 155.8 against 152.9 Msamples/s at 32 M; at 16 M two views 146.8 against 144.3).
// req_views: tray_scene_set_wavefront (0 = this rule); TRAYHIP_WF_PIPES overrides
inline uint32_t view_count(uint32_t n_chunks, uint32_t req_views) {
    uint32_t n_views = n_chunks >= (24u << 20) / TR_BLOCK ? 1u : 2u;
    if (req_views) n_views = std::min<uint32_t>(WF_PIPES_MAX, req_views);
    if (const char* e = getenv("TRAYHIP_WF_PIPES")) n_views = (uint32_t)std::max(1, std::min(WF_PIPES_MAX, atoi(e)));
    return std::max(1u, std::min(n_views, n_chunks / WF_SEGS));   // (a view of a few chunks would only add launches)
}
// every chunk needs at most (a work item's samples / 4 rounded up) x (max_depth + 2) rounds per work item, plus one round per item switch
// (WF_FOLD_C: a vertex with a stage C ray takes two rounds); n: the launch's samples per pixel, cut into 2^slice_shift work items per tile
inline uint64_t max_rounds(uint32_t n_items, uint32_t n_chunks, uint32_t n, uint32_t slice_shift, uint32_t max_depth) {
    const uint64_t items_per_chunk = ((uint64_t)n_items + n_chunks - 1u) / n_chunks;
    return items_per_chunk * (((uint64_t)((n + (1u << slice_shift) - 1u) >> slice_shift) + 3) / 4 * ((WF_FOLD_C ? 2u : 1u) * max_depth + 3) + 4) + 2 * WF_POLL;
}
// launches per round and view as tray_last_timing counts them (nominal: a kind-pure launch per material kind present comes on top in both forms)
inline uint32_t nominal_launches(uint32_t bin_stages) { return (WF_FOLD_C ? 8u : 10u) + ((bin_stages & 1u) ? 2u : 0u) + ((bin_stages & 2u) ? 2u : 0u); }

// ---- the buffers' shape, for a pool of pool_chunks chunks and up to WF_PIPES_MAX views

enum Queue : uint32_t { QA, QB, QC, QR };   // the ray queues of stages A, B, C (an entry is the ray: WF_RAY_WORDS words) and the regeneration queue (slot indices)

// The queue buffer holds the four queue kinds one after the other, each with room for every view's segments, then the views' control words. A view's
// segments are sized for its own chunks: WF_SEGS * TR_BLOCK entries of rounding per view and queue on top of the pool's own WF_SEGS * seg_cap.
struct Layout {
    uint64_t q_total;           // entries of one queue kind over all views
    uint64_t q_word[4];         // first word of queue kind A, B, C, R in the queue buffer
    uint64_t qctl_word;         // ... and of view 0's control words (WF_QCTL_WORDS per view)
    uint64_t bin_ctl_words;     // ray binning, per view: for stage A and stage B the histogram and the cursors of every segment's bins
    uint64_t kind_entries;      // shading queues of the material sort (slot indices), one per material kind, over all views
    uint64_t ovf_entries;       // overflow stack entries per view (the views' traversal kernels overlap)
    uint64_t queue_bytes, bin_ctl_bytes, kind_bytes, ovf_bytes;   // the four allocations
};
// full_depth / lds_depth: stack entries per lane of the dynamic-fetch traversal, and how many of them lie in LDS; n_blocks_trace: its persistent grid
inline Layout layout(uint32_t pool_chunks, uint32_t full_depth, uint32_t lds_depth, uint32_t n_blocks_trace) {
    Layout l;
    l.q_total = (uint64_t)WF_SEGS * wf_seg_cap(pool_chunks) + (uint64_t)WF_PIPES_MAX * WF_SEGS * TR_BLOCK;
    for (uint32_t q = 0; q < 4u; ++q) l.q_word[q] = (uint64_t)q * WF_RAY_WORDS * l.q_total;
    l.qctl_word = l.q_word[QR] + l.q_total;
    l.bin_ctl_words = (uint64_t)2u * 2u * WF_SEGS * WF_BINS;
    l.kind_entries = (uint64_t)WF_MAT_KINDS * l.q_total;
    l.ovf_entries = (uint64_t)(full_depth - lds_depth + 1u) * n_blocks_trace * TR_BLOCK;
    l.queue_bytes = (l.qctl_word + (uint64_t)WF_PIPES_MAX * WF_QCTL_WORDS) * sizeof(uint32_t);
    l.bin_ctl_bytes = (uint64_t)WF_PIPES_MAX * l.bin_ctl_words * sizeof(uint32_t);
    l.kind_bytes = l.kind_entries * sizeof(uint32_t);
    l.ovf_bytes = (uint64_t)WF_PIPES_MAX * l.ovf_entries * sizeof(uint32_t);
    return l;
}

// A VIEW of the wavefront buffers: a range of the pool's chunks with queues, control words and overflow columns of its own. The schedule runs its views
// each on its own stream: every stage kernel ends with the tail of its slowest rays (trace C is nearly all tail: a few thousand rays, ~600 us for the
// longest chain of dependent fetches), and while one view's kernel drains, the workgroups it frees run the other view's kernels. The views share the
// tile counter, so the split does not unbalance them.
struct View {
    uint32_t first_chunk, n_chunks, seg_cap;   // seg_cap: wf_seg_cap of the view's own chunks
    uint64_t q_off;                            // the view's first entry within every queue kind
    uint64_t qctl_word, bin_ctl_word, ovf_entry;   // where its control words, bin-control words and overflow columns begin in their buffers
};
// view k of n_views over the n_chunks chunks in use: equal shares, one after the other
inline View view(const Layout& l, uint32_t k, uint32_t n_views, uint32_t n_chunks) {
    auto first = [&](uint32_t j) { return (uint32_t)((uint64_t)n_chunks * j / n_views); };
    View v;
    v.first_chunk = first(k);
    v.n_chunks = first(k + 1u) - v.first_chunk;
    v.seg_cap = wf_seg_cap(v.n_chunks);
    v.q_off = 0;
    for (uint32_t j = 0; j < k; ++j) v.q_off += (uint64_t)WF_SEGS * wf_seg_cap(first(j + 1u) - first(j));
    v.qctl_word = l.qctl_word + (uint64_t)k * WF_QCTL_WORDS;
    v.bin_ctl_word = (uint64_t)k * l.bin_ctl_words;
    v.ovf_entry = (uint64_t)k * l.ovf_entries;
    return v;
}
// a view's pointers into the four allocations (kind_queues: null for scenes that shade unsorted; bin_ctl: null without the binning buffer)
struct Buffers {
    uint32_t* q[4];   // by Queue
    uint32_t *qctl, *kq, *bin_ctl, *overflow;
};
inline Buffers buffers(const Layout& l, const View& v, uint32_t* queues, uint32_t* kind_queues, uint32_t* bin_ctl, uint32_t* overflow) {
    Buffers b;
    for (uint32_t q = 0; q < 4u; ++q) b.q[q] = queues + l.q_word[q] + (q == QR ? 1u : WF_RAY_WORDS) * v.q_off;
    b.qctl = queues + v.qctl_word;
    b.kq = kind_queues ? kind_queues + (uint64_t)WF_MAT_KINDS * v.q_off : nullptr;
    b.bin_ctl = bin_ctl ? bin_ctl + v.bin_ctl_word : nullptr;
    b.overflow = overflow + v.ovf_entry;
    return b;
}

// ---- one round

struct RoundCfg {
    bool sorted;             // the scene's materials are sorted by kind (no textured ones): kind-pure shading over the material sort's queues
    bool fused;              // fused_wanted()
    uint32_t bin_stages;     // bin_stages_wanted()
    bool bin_ctl;            // the binning buffer exists
    uint32_t kinds_present;  // bit per TRAY_MAT_* kind among the scene's materials
};
// Fused shading (wavefront.h: k_wf_sort + k_wf_shade_kind; scenes whose materials are sorted by kind, i.e. without textured ones): the vertex is shaded in
// ONE kernel between the two traversals, its light term pending until the occlusion ray is traced; TRAYHIP_WF_FUSED=0: the two-kernel form of rounds 2-5
inline bool fused(const RoundCfg& c) { return c.sorted && c.fused && WF_FOLD_C; }
// ray binning (wavefront.h: k_wf_bin_hist / k_wf_bin_scatter) before stage S: the stage's queue, every segment sorted by (origin cell, direction octant)
// into the ray queue that is idle during the stage -- C's for stage A (WF_FOLD_C: nobody fills it), A's for stage B (consumed by then) --, which is what
// the traversal then draws from; the fallback records go where they went (B's buffer during A, C's during B: the sorted copy is consumed by then)
inline bool binned(const RoundCfg& c, uint32_t stage) { return WF_FOLD_C && c.bin_ctl && (c.bin_stages & (1u << stage)); }
// (WF_FOLD_C: stage C rays travel with the next round's stage A rays, no queue and no launch of their own -- the query kernels get no queue C)
constexpr bool kStageC = !WF_FOLD_C;

// f(integral_constant K) for every material kind present, in TRAY_MAT_* order
template <int K = 0, class F>
inline void each_kind(uint32_t kinds_present, F&& f) {
    if constexpr (K < WF_MAT_KINDS) {
        if (kinds_present & (1u << K)) f(std::integral_constant<int, K>{});
        each_kind<K + 1>(kinds_present, f);
    }
}

// One round of the wavefront schedule: advance -> regen -> trace A -> begin -> trace B -> query -> trace C (compacted ray queues, persistent
// traversal with dynamic fetch, kind-pure shading over the material sort's queues; scenes with textured materials, whose lobes exist per hit
// only, shade unsorted in the one instantiation that lowers them). Ops names the kernels, one member per launch group, and keeps its grids:
//   advance<ANIM>() (the whole frame or the launch's sample range), regen<ANIM>(), bin<S>(from, to), clear_qctl(), sort(), shade_kind<ANIM, K>(),
//   begin<ANIM>(), query_kind<ANIM, K>(stage_c), query<ANIM>(stage_c),
//   trace<S, ANIM>(from, fallback, fused): the traversal of stage S over queue `from`, then the few-thread kernel that traces the rays it handed over
//   to the reference's binary traversal: direction components that are zero / denormal / not finite -- normally none, the kernel reads one word and
//   exits. The deferred rays' records go to the buffer of a ray queue that is idle during the stage: B's during A, C's during B, B's during C.
template <int ANIM, class Ops>
inline void round(Ops& ops, const RoundCfg& c) {
    ops.template advance<ANIM>();
    ops.template regen<ANIM>();
    if (binned(c, 0u)) { ops.template bin<0>(QA, QC); ops.template trace<0, ANIM>(QC, QB, 0u); }
    else ops.template trace<0, ANIM>(QA, QB, 0u);
    // the control words of every queue are cleared HERE, between the traversal of stage A and the first shading kernel: queue A, its cursors, the
    // regeneration queue and stage A's fallback counter are consumed, stage B's and the material kinds' are not produced yet -- and the count of
    // queue A must survive from the query kernels below (which append the NEXT round's continuation rays) to the next round's traversal
    (void)ops.clear_qctl();
    if (fused(c)) {
        ops.sort();
        each_kind(c.kinds_present, [&](auto k) { ops.template shade_kind<ANIM, decltype(k)::value>(); });
        ops.template trace<1, ANIM>(QB, QC, 1u);
        return;
    }
    ops.template begin<ANIM>();
    if (binned(c, 1u)) { ops.template bin<1>(QB, QA); ops.template trace<1, ANIM>(QA, QC, 0u); }
    else ops.template trace<1, ANIM>(QB, QC, 0u);
    if (c.sorted) each_kind(c.kinds_present, [&](auto k) { ops.template query_kind<ANIM, decltype(k)::value>(kStageC); });   // one launch per material kind the scene contains
    else ops.template query<ANIM>(kStageC);
    if (WF_FOLD_C) return;
    // (builds without WF_FOLD_C: the deferred rays of stage C go to B's buffer -- A's holds the next round's continuation rays by now)
    ops.template trace<2, ANIM>(QC, QB, 0u);
}

// ---- the loop

enum Ended { kDone, kFailed, kNotTerminated };
// Rounds over the views until `poll` reads that every work item is done: each view's control words are cleared once (later: inside the round), the
// bin-control words before every round that bins; poll() (0: go on, 1: all done, < 0: failed) is asked every poll_interval rounds. views[k]: the Ops
// of view k, whose clear_qctl() / clear_bin_ctl() return 0 or a failure's code. *rounds: the rounds that ran.
template <int ANIM, class Ops, class Poll>
inline Ended run(Ops* views, uint32_t n_views, const RoundCfg& c, uint64_t max_rounds, uint32_t poll_interval, Poll&& poll, uint64_t* rounds) {
    *rounds = 0;
    for (uint32_t k = 0; k < n_views; ++k)
        if (views[k].clear_qctl() != 0) return kFailed;
    for (uint64_t r = 0;; ++r) {
        for (uint32_t k = 0; k < n_views; ++k) {
            if (c.bin_ctl && c.bin_stages && views[k].clear_bin_ctl() != 0) return kFailed;
            round<ANIM>(views[k], c);
        }
        *rounds = r + 1u;
        int done = 0;
        if (r % poll_interval == poll_interval - 1u && (done = poll()) < 0) return kFailed;
        if (r > max_rounds) return kNotTerminated;
        if (done) return kDone;
    }
}

}  // namespace tr_wfplan
