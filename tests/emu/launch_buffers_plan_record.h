// TEST INFRASTRUCTURE ONLY: tray_rust_amd/csrc/hip/launch_buffers_plan.h's sizes, rules and procedures by number, for tests/test_launch_buffers_plan.py
// (these are exports of libtrayemu.so: emu_kernels.cpp includes this file) and for the stand-alone launch_buffers_plan_check.cpp. ScriptedOps allocates
// nothing: it reports a free-byte figure (or that it has none), grants what is no larger than a largest grantable allocation -- hipMalloc under the
// stand-in runtime of tests/stubs/fakehip.c with FAKEHIP_FREE_BYTES and FAKEHIP_MALLOC_MAX --, logs every call and keeps the set of live grants.
// Include after kernels.hip, wavefront_plan.h and launch_buffers_plan.h.
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace lb_record {
namespace lp = tr_lbplan;

enum Call : uint32_t { kFreeBytes, kGrantCache, kGrantTable, kGrantPool, kDrop, kSynchronise, kTableBuild, kTableWait, kRefusal, kNoPool, kCacheShort };
struct Entry { uint64_t call, a, b; };   // a: lanes / slots / parts / stride; b: bytes, or the outcome
struct Grant { unsigned part; uint64_t bytes; uint32_t drops; };

struct ScriptedOps {
    uint64_t free_b = (uint64_t)4 << 30;
    bool free_known = true;
    uint64_t max_grant = ~(uint64_t)0;                       // the largest single allocation that is granted
    uint32_t quad_stack_words = 24, trace_blocks = 512;      // what the pool's queue and overflow buffers are sized by besides its slots
    int refuse = 0;                                          // refusal()'s answer
    std::vector<Entry> log;
    std::vector<Grant> grants;                               // every grant ever made
    int live[3] = {-1, -1, -1};                              // the live grant of the pool, the cache, the table: index into grants
    uint32_t misuse = 0;                                     // grants of a part that is live, drops of a part that is not

    void note(uint32_t call, uint64_t a = 0, uint64_t b = 0) { log.push_back({call, a, b}); }
    static int index(unsigned part) { return part == lp::kPool ? 0 : part == lp::kCache ? 1 : 2; }
    void grant(unsigned part, uint64_t bytes) {
        misuse += live[index(part)] >= 0;
        live[index(part)] = (int)grants.size();
        grants.push_back({part, bytes, 0u});
    }

    bool free_bytes(uint64_t* out) { note(kFreeBytes, free_known, free_b); *out = free_b; return free_known; }
    bool grant_cache(uint32_t lanes, uint64_t bytes) {
        const bool ok = bytes <= max_grant;
        note(kGrantCache, lanes, ok ? bytes : 0);
        if (ok) grant(lp::kCache, bytes);
        return ok;
    }
    bool grant_table(uint64_t bytes) {
        const bool ok = bytes <= max_grant;
        note(kGrantTable, bytes, ok);
        if (ok) grant(lp::kTable, bytes);
        return ok;
    }
    // the allocations of the library's grant_pool, in its order; one refused: nothing stays
    int grant_pool(uint32_t n_slots) {
        const uint32_t n_chunks = n_slots / TR_BLOCK, full = lp::trace_full_depth(quad_stack_words);
        const tr_wfplan::Layout lay = tr_wfplan::layout(n_chunks, full, lp::trace_lds_depth(full), trace_blocks);
        const uint64_t sizes[] = {lp::pool_bytes(n_slots), lp::chunk_bytes(n_chunks), lp::bin_bytes(n_chunks), 2 * sizeof(uint32_t),
                                  lay.queue_bytes, lay.bin_ctl_bytes, lay.kind_bytes, lay.ovf_bytes};
        uint64_t total = 0;
        bool ok = true;
        for (const uint64_t b : sizes) { ok = ok && b <= max_grant; total += b; }
        note(kGrantPool, n_slots, ok);
        if (ok) grant(lp::kPool, total);
        return ok ? TRAY_OK : TRAY_E_NOMEM;
    }
    void drop(unsigned what) {
        note(kDrop, what);
        for (const unsigned part : {(unsigned)lp::kPool, (unsigned)lp::kCache, (unsigned)lp::kTable}) {
            if (!(what & part)) continue;
            int& l = live[index(part)];
            if (l < 0) { ++misuse; continue; }
            ++grants[(size_t)l].drops;
            l = -1;
        }
    }
    int synchronise() { note(kSynchronise); return 0; }
    int table_build(uint32_t stride) { note(kTableBuild, stride); return 0; }
    int table_wait() { note(kTableWait); return 0; }
    int refusal() { note(kRefusal, (uint64_t)(int64_t)refuse); return refuse; }
    void no_pool(uint32_t n_slots) { note(kNoPool, n_slots); }
    void cache_short(uint32_t pool_slots, uint32_t lanes) { note(kCacheShort, pool_slots, lanes); }
};

// a device scene's launch buffers as the plan sees them: the facts, the state, the Ops
struct Session {
    lp::Facts f{};
    lp::State st;
    ScriptedOps ops;

    int frame() { bool kept; return lp::frame(ops, st, f, &kept); }   // tray_scene_create / tray_scene_update_frame
    int prepare(uint64_t samples) { return lp::prepare(ops, st, f, samples); }   // a render call
    void set_wavefront(uint32_t req_slots) {   // tray_scene_set_wavefront
        const bool goes = lp::wish_changed(st, f.n_tiles, f.req_slots, req_slots);
        f.req_slots = req_slots;
        if (goes) { (void)ops.synchronise(); lp::drop_pool(ops, st); }
    }
    bool reads_cache() const { return f.wavefront && !st.last_used_table && f.n_moving != 0u; }

    // every grant is owned by the state or was dropped exactly once, and nothing dropped is still named by the state: "" or what is wrong
    std::string owned() const {
        if (ops.misuse) return "a part was granted twice or dropped while not live";
        const bool named[3] = {st.pool, st.cache, st.table};
        for (int p = 0; p < 3; ++p)
            if (named[p] != (ops.live[p] >= 0)) return std::string("the state and the live grants differ on the ") + (p == 0 ? "pool" : p == 1 ? "cache" : "table");
        for (size_t g = 0; g < ops.grants.size(); ++g) {
            const bool is_live = ops.live[ScriptedOps::index(ops.grants[g].part)] == (int)g;
            if (ops.grants[g].drops != (is_live ? 0u : 1u)) return "a grant is neither live nor dropped exactly once";
        }
        if (st.cache && ops.grants[(size_t)ops.live[1]].bytes != st.cache_bytes) return "the cache's bytes are not the granted ones";
        if (st.table && ops.grants[(size_t)ops.live[2]].bytes != lp::table_bytes(st.table_cap)) return "the table's bytes are not the granted ones";
        return "";
    }
    // after a prepare that returned TRAY_OK: "" or the invariant of launch_buffers_plan.h that does not hold
    std::string launchable() const {
        if (reads_cache() && !(st.cache && st.cache_lanes >= st.pool_slots && st.cache_bytes >= lp::cache_bytes(f.n_moving, true, st.pool_slots)))
            return "a launch that reads the cache has no record for every pool slot";
        if (f.wavefront && !(st.pool && st.pool_slots != 0u && st.pool_slots % TR_BLOCK == 0u && st.pool_slots <= lp::slot_wish(f.n_tiles, f.req_slots)))
            return "the pool's slots are no multiple of TR_BLOCK or more than the wish";
        if (st.last_used_table && !(st.table && st.table_built && st.table_stride != 0u && st.table_stride <= st.table_cap))
            return "a table launch without a built table of stride <= cap";
        return "";
    }
};

// The invariant sweep: prepare over free bytes x largest grant x table request x sample count x movers x film x prior state (built with the memory
// the prior launches had), then a second prepare with the table request turned round -- ADVICE round 6's sequence is the case "a per-path launch with
// little memory, tray_scene_set_wavefront, a table launch with much, table off". Returns the cases run, *failures their number that broke an invariant,
// first: the first one's description.
inline uint64_t sweep(uint64_t* failures, std::string* first) {
    const uint64_t GiB = (uint64_t)1 << 30, MiB = (uint64_t)1 << 20, none = ~(uint64_t)0;
    enum Prior { kFresh, kPerPath, kTableLaunch, kPerPathDrop, kTableDrop, kPerPathUpdate, kTableUpdate, kPriors };
    uint64_t cases = 0;
    *failures = 0;
    for (const uint64_t free_b : {(uint64_t)0, GiB, 3 * GiB, 4 * GiB, 256 * GiB, none})   // (none: the device cannot be asked)
    for (const uint64_t max_grant : {16 * MiB, 64 * MiB, 768 * MiB, GiB, none})
    for (const int table_req : {-1, 0, 1})
    for (const uint64_t samples : {(uint64_t)65536, (uint64_t)XF_TABLE_MIN_SAMPLES})
    for (const uint32_t movers : {0u, 4u})
    for (const uint32_t n_tiles : {64u, 32400u})
    for (const uint64_t prior_free : {GiB, 256 * GiB})
    for (int prior = 0; prior < kPriors; ++prior) {
        Session s;
        s.f = lp::Facts{n_tiles, 1024u, true, movers != 0u, movers, 8192u, 24u, movers ? movers + 3u : 0u, movers != 0u, 0u, -1};
        s.ops.free_b = prior_free;
        char what[256];
        std::snprintf(what, sizeof what, "free %llu, largest grant %llu, table request %d, %llu samples, %u movers, %u tiles, prior %d with %llu free",
                      (unsigned long long)free_b, (unsigned long long)max_grant, table_req, (unsigned long long)samples, movers, n_tiles, prior, (unsigned long long)prior_free);
        auto fail = [&](const char* when, const std::string& why) {
            if (why.empty()) return;
            if (!(*failures)++) *first = std::string(what) + ", " + when + ": " + why;
        };
        int rc = s.frame();
        if (prior != kFresh) {
            if (prior == kPerPathDrop || prior == kTableDrop) s.set_wavefront(32768u);
            s.f.table_req = (prior == kPerPath || prior == kPerPathDrop || prior == kPerPathUpdate) ? 0 : 1;
            if (rc == TRAY_OK) rc = s.prepare(65536u);
            if (rc == TRAY_OK) fail("after the prior launch", s.launchable());
            if (prior == kPerPathDrop || prior == kTableDrop) s.set_wavefront(1u << 26);   // (a wish far above a cache budgeted with little memory)
            if (prior == kPerPathUpdate || prior == kTableUpdate) rc = s.frame();
        }
        fail("before the case", s.owned());
        s.ops.free_known = free_b != none; s.ops.free_b = free_b; s.ops.max_grant = max_grant;
        s.f.table_req = table_req;
        rc = s.prepare(samples);
        if (rc == TRAY_OK) fail("after prepare", s.launchable());
        fail("after prepare", s.owned());
        s.f.table_req = table_req == 0 ? 1 : 0;
        rc = s.prepare(samples);
        if (rc == TRAY_OK) fail("after the second prepare", s.launchable());
        fail("after the second prepare", s.owned());
        ++cases;
    }
    return cases;
}

}  // namespace lb_record

extern "C" {

// TR_BLOCK, TR_XF_REC, TR_XF_WORDS, F_COUNT, WF_RAY_WORDS, WF_MAT_KINDS, ROWBIN_SIZE, sizeof(WfChunk), WF_MAX_SLICES, WF_TRACE_WAVES, WF_SLOTS,
// XF_TABLE_MIN_SAMPLES, the time indices, TRAY_E_NOMEM, TRAY_E_DEVICE (as 64-bit two's complement)
void emu_lb_plan_constants(uint64_t* out) {
    const uint64_t c[] = {TR_BLOCK, TR_XF_REC, TR_XF_WORDS, F_COUNT, WF_RAY_WORDS, WF_MAT_KINDS, ROWBIN_SIZE, sizeof(WfChunk), WF_MAX_SLICES, WF_TRACE_WAVES, WF_SLOTS,
                          XF_TABLE_MIN_SAMPLES, tr_lbplan::kTimeIndices, (uint64_t)(int64_t)TRAY_E_NOMEM, (uint64_t)(int64_t)TRAY_E_DEVICE};
    for (uint32_t i = 0; i < sizeof c / sizeof *c; ++i) out[i] = c[i];
}
// pool bytes, schedule bytes per slot, chunk bytes, bin bytes, cache bytes, table bytes
void emu_lb_plan_sizes(uint32_t n_slots, uint32_t n_chunks, uint32_t n_moving, int wavefront, uint32_t lanes, uint32_t cap, uint64_t* out) {
    const uint64_t f[] = {tr_lbplan::pool_bytes(n_slots), tr_lbplan::schedule_bytes_per_slot(), tr_lbplan::chunk_bytes(n_chunks), tr_lbplan::bin_bytes(n_chunks),
                          tr_lbplan::cache_bytes(n_moving, wavefront != 0, lanes), tr_lbplan::table_bytes(cap)};
    for (uint32_t i = 0; i < sizeof f / sizeof *f; ++i) out[i] = f[i];
}
uint32_t emu_lb_plan_slot_wish(uint32_t n_tiles, uint32_t req_slots) { return tr_lbplan::slot_wish(n_tiles, req_slots); }
uint32_t emu_lb_plan_slot_fit(uint32_t n_tiles, uint64_t slots, uint64_t free_b, uint32_t req_slots) { return tr_lbplan::slot_fit(n_tiles, slots, free_b, req_slots); }
uint32_t emu_lb_plan_cache_budget(uint32_t n_tiles, uint32_t n_moving, uint64_t free_b) { return tr_lbplan::cache_budget(n_tiles, n_moving, free_b); }
int emu_lb_plan_table_wanted(int table_req, uint64_t samples, int built, int exists) {
    tr_lbplan::State b;
    b.table_built = built != 0; b.table = exists != 0;
    return tr_lbplan::table_wanted(table_req, samples, b) ? 1 : 0;
}
// full depth, LDS depth of the dynamic-fetch traversal's stacks
void emu_lb_plan_trace_depths(uint32_t quad_stack_words, uint32_t* out) {
    out[0] = tr_lbplan::trace_full_depth(quad_stack_words);
    out[1] = tr_lbplan::trace_lds_depth(out[0]);
}
int emu_lb_plan_wish_changed(int pool, uint32_t n_tiles, uint32_t req_before, uint32_t req_after) {
    tr_lbplan::State b;
    b.pool = pool != 0;
    return tr_lbplan::wish_changed(b, n_tiles, req_before, req_after) ? 1 : 0;
}

// a Session; facts: the eleven of tr_lbplan::Facts in the struct's order
void* emu_lb_plan_new() { return new lb_record::Session(); }
void emu_lb_plan_delete(void* h) { delete static_cast<lb_record::Session*>(h); }
void emu_lb_plan_facts(void* h, const int64_t* v) {
    static_cast<lb_record::Session*>(h)->f = tr_lbplan::Facts{(uint32_t)v[0], (uint32_t)v[1], v[2] != 0, v[3] != 0, (uint32_t)v[4], (uint32_t)v[5], (uint32_t)v[6],
                                                             (uint32_t)v[7], v[8] != 0, (uint32_t)v[9], (int)v[10]};
}
void emu_lb_plan_table_request(void* h, int mode) { static_cast<lb_record::Session*>(h)->f.table_req = mode; }
void emu_lb_plan_memory(void* h, uint64_t free_b, int free_known, uint64_t max_grant) {
    lb_record::ScriptedOps& o = static_cast<lb_record::Session*>(h)->ops;
    o.free_b = free_b; o.free_known = free_known != 0; o.max_grant = max_grant;
}
int emu_lb_plan_frame(void* h) { return static_cast<lb_record::Session*>(h)->frame(); }
int emu_lb_plan_prepare(void* h, uint64_t samples) { return static_cast<lb_record::Session*>(h)->prepare(samples); }
void emu_lb_plan_set_wavefront(void* h, uint32_t req_slots) { static_cast<lb_record::Session*>(h)->set_wavefront(req_slots); }
// what tray_last_schedule reports of the state (pool slots, cache bytes, table bytes, the last launch read the table), then cache lanes, table stride,
// table cap, table built, the pool came out smaller than asked for
void emu_lb_plan_state(void* h, uint64_t* out) {
    const tr_lbplan::State& b = static_cast<lb_record::Session*>(h)->st;
    const uint64_t f[] = {b.pool_slots, b.cache_bytes, tr_lbplan::table_bytes(b.table_cap), b.last_used_table, b.cache_lanes, b.table_stride, b.table_cap,
                          b.table_built, b.wf_shrunk};
    for (uint32_t i = 0; i < sizeof f / sizeof *f; ++i) out[i] = f[i];
}
// "" (returns 0) or the first invariant that does not hold, as text; launched: the last prepare returned TRAY_OK
uint32_t emu_lb_plan_broken(void* h, int launched, char* msg, uint32_t cap) {
    const lb_record::Session& s = *static_cast<lb_record::Session*>(h);
    std::string why = s.owned();
    if (why.empty() && launched) why = s.launchable();
    std::snprintf(msg, cap, "%s", why.c_str());
    return why.empty() ? 0u : 1u;
}
// the Ops' calls so far, three words each (lb_record::Entry), the first `cap` of them; returns their number
uint32_t emu_lb_plan_log(void* h, uint64_t* out, uint32_t cap) {
    const std::vector<lb_record::Entry>& l = static_cast<lb_record::Session*>(h)->ops.log;
    for (uint32_t i = 0; i < l.size() && i < cap; ++i) { out[3u * i] = l[i].call; out[3u * i + 1u] = l[i].a; out[3u * i + 2u] = l[i].b; }
    return (uint32_t)l.size();
}
// lb_record::sweep: the cases run; *failures and the first failure's description
uint64_t emu_lb_plan_sweep(uint64_t* failures, char* msg, uint32_t cap) {
    std::string first;
    const uint64_t cases = lb_record::sweep(failures, &first);
    std::snprintf(msg, cap, "%s", first.c_str());
    return cases;
}

}  // extern "C"
