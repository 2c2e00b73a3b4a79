// TEST INFRASTRUCTURE ONLY: a stand-alone program that runs the host-only functions of csrc/hip/wavefront_plan.h -- the layout and every view of it over
// the pool sizes of tests/test_wavefront_plan.py, every round with a recording Ops, the loop with an Ops that launches nothing -- to be built with the host
// sanitizers and run by hand on a machine without a GPU (no test runs it):
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Wno-attributes -o /tmp/wavefront_plan_check wavefront_plan_check.cpp && /tmp/wavefront_plan_check
// Exit status 0: the views partition the chunks and stay inside the allocations, every round has the launches it should, and no sanitizer report.
#include "hip_emu.h"
#include "../../tray_rust_amd/csrc/hip/kernels.hip"
#include "../../tray_rust_amd/csrc/hip/wavefront_plan.h"
#include "wavefront_plan_record.h"

namespace trayh { void set_error(const std::string&) {} }

int main() {
    namespace wp = tr_wfplan;
    using namespace wf_record;
    int bad = 0;
    for (uint32_t pool : {1u, 63u, 64u, 65u, 70u, 128u, 4096u, 131072u, 1u << 20}) {
        const wp::Layout l = wp::layout(pool, 40u, 24u, 512u);
        bad += l.qctl_word != (3u * WF_RAY_WORDS + 1u) * l.q_total || l.queue_bytes != (l.qctl_word + (uint64_t)WF_PIPES_MAX * WF_QCTL_WORDS) * 4u;
        for (uint32_t used : {1u, std::max(1u, pool / 2u), pool})
            for (uint32_t want = 1; want <= WF_PIPES_MAX; ++want) {
                const uint32_t n_views = wp::view_count(used, want);
                uint32_t next_chunk = 0;
                uint64_t next_entry = 0;
                for (uint32_t k = 0; k < n_views; ++k) {
                    const wp::View v = wp::view(l, k, n_views, used);
                    bad += v.first_chunk != next_chunk || v.q_off != next_entry || v.seg_cap != wf_seg_cap(v.n_chunks);
                    next_chunk += v.n_chunks;
                    next_entry += (uint64_t)WF_SEGS * v.seg_cap;
                    bad += (v.qctl_word + WF_QCTL_WORDS) * 4u > l.queue_bytes || (v.bin_ctl_word + l.bin_ctl_words) * 4u > l.bin_ctl_bytes ||
                           (v.ovf_entry + l.ovf_entries) * 4u > l.ovf_bytes;
                }
                bad += next_chunk != used || next_entry > l.q_total;
            }
        std::printf("pool of %7u chunks: %llu entries per queue kind, queues %llu bytes%s\n", pool, (unsigned long long)l.q_total, (unsigned long long)l.queue_bytes,
                    bad ? " WRONG" : "");
    }
    {   // a small pool's pointers: the last word of each of a view's parts is written (the address sanitizer sees a write past an allocation)
        const wp::Layout l = wp::layout(130u, 12u, 8u, 3u);
        std::vector<uint32_t> queues(l.queue_bytes / 4u), kinds(l.kind_bytes / 4u), bin_ctl(l.bin_ctl_bytes / 4u), overflow(l.ovf_bytes / 4u);
        for (uint32_t k = 0; k < WF_PIPES_MAX; ++k) {
            const wp::View v = wp::view(l, k, WF_PIPES_MAX, 130u);
            const wp::Buffers b = wp::buffers(l, v, queues.data(), kinds.data(), bin_ctl.data(), overflow.data());
            const uint64_t entries = (uint64_t)WF_SEGS * v.seg_cap;
            for (uint32_t q = 0; q < 3u; ++q) b.q[q][WF_RAY_WORDS * entries - 1u] = k;
            b.q[wp::QR][entries - 1u] = k; b.qctl[WF_QCTL_WORDS - 1u] = k; b.kq[WF_MAT_KINDS * entries - 1u] = k;
            b.bin_ctl[l.bin_ctl_words - 1u] = k; b.overflow[l.ovf_entries - 1u] = k;
        }
    }
    // every round: the launches of its groups (bin and trace are two kernels, the control words' clear is none) against the nominal count, which has one
    // launch for the shading stage where the sorted forms have one per kind, and two per stage asked to be binned where the fused form never bins stage B
    for (int form = 0; form < 2; ++form)
        for (int sorted = 0; sorted < 2; ++sorted)
            for (uint32_t bins = 0; bins < 4u; ++bins)
                for (uint32_t kinds : {1u << 3, 0x45u, 0x7fu}) {
                    const wp::RoundCfg c{sorted != 0, form != 0, bins, true, kinds};
                    uint32_t launches = 0, kind_launches = 0;
                    for (const Launch& g : record_round(false, c)) {
                        launches += g.group == kBin || g.group == kTrace ? 2u : g.group == kClearQctl ? 0u : 1u;
                        kind_launches += g.group == kShadeKind || g.group == kQueryKind;
                    }
                    const uint32_t want = wp::nominal_launches(bins) - (sorted ? 1u : 0u) - (wp::fused(c) && (bins & 2u) ? 2u : 0u);
                    const bool wrong = launches - kind_launches != want || kind_launches != (sorted ? (uint32_t)__builtin_popcount(kinds) : 0u);
                    if (wrong) std::printf("WRONG fused %d sorted %d bins %u kinds %#x: %u launches, %u of them per kind\n", form, sorted, bins, kinds, launches, kind_launches);
                    bad += wrong;
                }
    // the loop: two views, "done" at the first poll; then a schedule that never ends
    RecordingOps views[2];
    uint64_t rounds = 0;
    const wp::RoundCfg c{true, true, 3u, true, 0x7fu};
    bad += wp::run<1>(views, 2u, c, 100u, WF_POLL, [] { return 1; }, &rounds) != wp::kDone || rounds != WF_POLL;
    bad += wp::run<0>(views, 2u, c, 40u, 1u, [] { return 0; }, &rounds) != wp::kNotTerminated || rounds != 42u;
    bad += wp::run<0>(views, 1u, c, 40u, 1u, [] { return -5; }, &rounds) != wp::kFailed || rounds != 1u;
    std::printf("%s\n", bad ? "FAILED" : "ok");
    return bad ? 1 : 0;
}
