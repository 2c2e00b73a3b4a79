// The launch buffers of a device scene on the host -- the wavefront pool with its queues, the per-path transform cache, the frame's transform table
// (dev_geom.h: xf_time_index): their sizes, the rules that size them, and the procedures that keep, drop and allocate them across launches,
// tray_scene_set_wavefront and frame updates. Host-only -- no HIP call, no device scene: device_api.hip runs the procedures with an Ops that makes the HIP
// calls, the tests (tests/emu/launch_buffers_plan_record.h) compile this header under g++ and run them with a scripted Ops, so every decision can be asked
// for without a GPU. Environment overrides that belong to a rule are read here, when the rule is asked. Include after kernels.hip and wavefront_plan.h
// (F_COUNT, WF_RAY_WORDS, WF_MAT_KINDS, ROWBIN_SIZE, WfChunk, TR_BLOCK, TR_XF_REC, TR_XF_WORDS, WF_TRACE_WAVES).
//
// What the procedures keep true (tests/test_launch_buffers_plan.py sweeps them): a wavefront launch that reads the per-path cache has a record for every
// pool slot -- the stage kernels index the cache by slot, so a pool larger than the cache is an out-of-bounds device access --; the pool's
// slots are whole chunks and no more than the wish; a launch that reads the table has a table built for this frame with no more records per time index
// than the buffer has room for; and a part the Ops granted is either named by the State or was dropped once.
//
// The Ops of the procedures:
//   bool free_bytes(uint64_t* out)          the device's free memory, or false: it cannot be asked (what that means is each caller's own, see below)
//   bool grant_cache(lanes, bytes)          the three allocations, granted or refused; grant_pool returns TRAY_OK, TRAY_E_NOMEM (the procedure halves and
//   bool grant_table(bytes)                 asks again) or another code (the procedure returns it); a refusal leaves nothing allocated
//   int  grant_pool(n_slots)
//   void drop(what)                         frees the parts named (kPool | kCache | kTable), which exist; no launch reads them any more
//   int  synchronise()                      waits for the device; 0 or a failure's code
//   int  table_build(stride), table_wait()  builds the frame's table on the launch's stream / makes the launch's stream wait for the build; 0 or a code
//   int  refusal()                          the schedule's own refusals of the scene, asked after cache or table and before the pool; 0 or a code
//   void no_pool(n_slots), cache_short(pool_slots, lanes)   the texts of the two failures that are the plan's own
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cstdlib>

#include "launch_rules.h"   // (WF_MAX_SLICES)

#ifndef WF_SLOTS
// Path pool slots the schedule asks for (capped by the film: a chunk of 256 per tile slice, 16 slices per tile -- 132.7 M at 1080p -- and by a third of the
// free memory; 0.47 KB per slot with queues and bins: 62 GB for a 1080p film on a 288 GB part). Every stage kernel ends with the tail of its slowest rays,
// and fewer, larger rounds pay it less often: 78 / 106 / 132 / 145 / 152 Msamples/s at 2 / 4 / 8 / 16 / 32 M slots (round 4); round 6, frame 64 / frame 127
// of the C5 stand-in at 512 spp: 237.6 / 169.7 at 32 M (4 slices per tile), 250 - 253 / 174 - 175 at 64 M (8), 256.6 / 177.7 at 128 M (16) -- as long as the
// pool's chunks and the work items are EQUAL in number (96 M slots under 16 slices: 242.0 / 170.5, a quarter of the chunks takes a second item while the others
// idle): launch_wavefront cuts tiles until the items fill the chunks and no further (profiles/r06_c5_pool_64m.txt, r06_c5_pool_128m.txt).
#define WF_SLOTS (128u << 20)
#endif
#ifndef XF_TABLE_MIN_SAMPLES
// The table when the launch needs every time index about twice: from 3e7 camera samples on, a 1080p frame at 16 spp (the build costs what 1.7e7
// evaluations cost, but takes 1.9 GB per moving instance)
#define XF_TABLE_MIN_SAMPLES 30000000ull
#endif

namespace tr_lbplan {

// ---- sizes

constexpr uint32_t kTimeIndices = 1u << 24;   // time indices of the transform table (dev_geom.h: xf_time_index)
constexpr uint32_t kMinSlots = 64u * TR_BLOCK;   // at least 64 chunks: below that the schedule cannot fill the chip

inline uint64_t pool_bytes(uint64_t n_slots) { return (uint64_t)F_COUNT * n_slots * sizeof(float); }
inline uint64_t chunk_bytes(uint32_t n_chunks) { return (uint64_t)n_chunks * sizeof(WfChunk); }
inline uint64_t bin_bytes(uint32_t n_chunks) { return (uint64_t)n_chunks * ROWBIN_SIZE * sizeof(float); }
// bytes of the schedule's buffers per pool slot (pool fields, three ray queues + regeneration queue, kind queues, fallback word, row bins per chunk)
inline uint64_t schedule_bytes_per_slot() {
    return (uint64_t)F_COUNT * sizeof(float) + (3 * WF_RAY_WORDS + 1) * sizeof(uint32_t) + WF_MAT_KINDS * sizeof(uint32_t) +
           ((uint64_t)ROWBIN_SIZE * sizeof(float) + sizeof(WfChunk)) / TR_BLOCK;
}
// a per-path transform cache of `lanes` paths (records of the wavefront schedule / rows of columns of the tile kernel: dev_anim.h)
inline uint64_t cache_bytes(uint32_t n_moving, bool wavefront, uint32_t lanes) {
    return (uint64_t)n_moving * (wavefront ? TR_XF_REC : TR_XF_WORDS) * lanes * sizeof(float);
}
// a transform table with room for `cap` records per time index (2.1 GB per moving instance)
inline uint64_t table_bytes(uint32_t cap) { return (uint64_t)kTimeIndices * cap * TR_XF_REC * sizeof(float); }

// ---- what the rules are functions of, and what the procedures keep

struct Facts {
    uint32_t n_tiles, tile_workgroups;   // the film's tiles; workgroups of the persistent tile kernel
    bool wavefront, animated;            // the schedule; something moves while the shutter is open
    uint32_t n_moving;                   // instances that move within the frame
    uint32_t stack_bytes, quad_stack_words;   // the scene's traversal stacks
    uint32_t xf_movable;                 // instances (+ camera) that ANY frame of the sequence can move
    bool camera_animated;
    uint32_t req_slots;                  // tray_scene_set_wavefront: 0 = the library's own rule
    int table_req;                       // tray_scene_set_transform_table: -1 = by the launch's sample count, 0 = never, 1 = always
};
enum : unsigned { kPool = 1u, kCache = 2u, kTable = 4u, kAll = 7u };
struct State {
    bool wavefront = false;              // the schedule the cache's layout and the pool were made for
    bool pool = false;                   // the pool and every buffer that goes with it exist
    uint32_t pool_slots = 0;
    uint32_t pool_stack_bytes = 0, pool_quad_stack_words = 0;   // the traversal stacks and ...
    bool pool_animated = false;          // ... kernels the pool's buffers were sized for
    bool wf_shrunk = false;              // the pool came out smaller than asked for (allocation failed, halved): frame updates keep it
    bool cache = false;
    uint64_t cache_bytes = 0;
    uint32_t cache_lanes = 0;            // paths the cache has room for; for a wavefront cache that does not exist yet: its budget (fit)
    bool table = false;
    uint32_t table_stride = 0, table_cap = 0;   // records per time index in use / room for (the next frames of a sequence may move more instances)
    bool table_built = false;            // ... for THIS frame (a frame update hands the buffer on, the frame's first launch that wants the table builds it)
    bool last_used_table = false;        // the last launch read the table
    bool owns_any() const { return pool || cache || table; }
};

// ---- rules

// what `req_slots`, the environment or the default ask for, before memory is looked at
inline uint32_t slot_wish(uint32_t n_tiles, uint32_t req_slots) {
    uint32_t n_slots = WF_SLOTS;
    if (req_slots) n_slots = std::max<uint32_t>(req_slots, kMinSlots) / TR_BLOCK * TR_BLOCK;   // tray_scene_set_wavefront
    if (const char* e = getenv("TRAYHIP_WF_SLOTS")) n_slots = (uint32_t)std::max(256l, atol(e)) / TR_BLOCK * TR_BLOCK;
    const uint64_t by_tiles = (uint64_t)std::max<uint32_t>(n_tiles, 1u) * TR_BLOCK * WF_MAX_SLICES;   // (a tile's samples can be cut into that many work items: launch_wavefront)
    return (uint32_t)std::min<uint64_t>(n_slots, by_tiles);
}
// `slots` within the share of the memory the pool may take, cut to the round-6 shape; free_b: what counts as free (the device's + what a frame update reclaims)
inline uint32_t slot_fit(uint32_t n_tiles, uint64_t slots, uint64_t free_b, uint32_t req_slots) {
    // the pool with its queues and bins (~0.47 KB per slot: 15 GB at 32 M) stays within a third of what is free now -- static scenes too
    // (a host that keeps several device scenes gets pools that fit beside each other; prepare halves on top if the allocation is refused)
    {
        const uint64_t fit = free_b / 3u / schedule_bytes_per_slot() / TR_BLOCK * TR_BLOCK;
        slots = std::min<uint64_t>(slots, std::max<uint64_t>(fit, kMinSlots));
    }
    // (round 6) the schedule is fastest with ONE work item per chunk (profiles/r06_c5_pool_128m.txt: 96 M slots under 16 slices per tile lose to 64 M under 8), so a
    // pool that memory cut below the film's 16 slices per tile is cut further to the next tiles x 256 x 2^k below it -- never to less than one chunk per tile
    {
        const uint64_t per_tile_level = (uint64_t)std::max<uint32_t>(n_tiles, 1u) * TR_BLOCK;
        if (slots > per_tile_level && !req_slots && !getenv("TRAYHIP_WF_SLOTS")) {
            uint64_t fit = per_tile_level;
            while (fit * 2u <= slots && fit * 2u <= per_tile_level * WF_MAX_SLICES) fit *= 2u;
            slots = fit;
        }
    }
    return (uint32_t)slots;
}
// The lanes of a moving scene's per-path transform cache (the largest pool a launch that reads it can have): the pool's rule, and the cache (112 B per slot
// and moving instance) within two fifths of free_b (the C5 stand-in has 2 .. 11 moving instances, 7 .. 39 GB at 32 M slots); TRAYHIP_XF_CACHE_BYTES
// overrides the two fifths. The library's rule and the environment alone: tray_scene_set_wavefront bounds the pool, not the cache.
inline uint32_t cache_budget(uint32_t n_tiles, uint32_t n_moving, uint64_t free_b) {
    uint64_t budget = free_b / 5 * 2;
    if (const char* e = getenv("TRAYHIP_XF_CACHE_BYTES")) budget = (uint64_t)std::max(0ll, atoll(e));
    const uint64_t per_slot = (uint64_t)n_moving * TR_XF_REC * sizeof(float);
    const uint64_t fit = budget / per_slot / TR_BLOCK * TR_BLOCK;
    const uint64_t slots = std::min<uint64_t>(slot_wish(n_tiles, 0u), std::max<uint64_t>(fit, kMinSlots));
    return slot_fit(n_tiles, slots, free_b, 0u);
}
// whether a launch of `samples` camera samples reads the table: as tray_scene_set_transform_table or TRAYHIP_XF_TABLE say, else from XF_TABLE_MIN_SAMPLES
// on, for every later launch of the frame and for the frames of a sequence that rendered through it
inline bool table_wanted(int table_req, uint64_t samples, const State& b) {
    int want = table_req;
    if (const char* e = getenv("TRAYHIP_XF_TABLE")) want = atoi(e) != 0 ? 1 : 0;
    if (want < 0) want = (samples >= XF_TABLE_MIN_SAMPLES || b.table_built || b.table) ? 1 : 0;
    return want != 0;
}
// Stack entries per lane of the dynamic-fetch traversal (a node on its stack is two words: descriptor and entry distance; up to three per expanded
// record), and how many of them lie in LDS: such that WF_TRACE_WAVES workgroups (4 waves each = one wave per SIMD) fit in the CU's 160 KB;
// TRAYHIP_WF_LDS_DEPTH overrides
inline uint32_t trace_full_depth(uint32_t quad_stack_words) { return std::max(quad_stack_words, 8u); }
inline uint32_t trace_lds_depth(uint32_t full_depth) {
    uint32_t lds_depth = std::min<uint32_t>(full_depth, (160u * 1024u / WF_TRACE_WAVES) / (TR_BLOCK * (uint32_t)sizeof(uint32_t)));
    if (const char* e = getenv("TRAYHIP_WF_LDS_DEPTH")) lds_depth = std::min<uint32_t>(full_depth, (uint32_t)std::max(1, atoi(e)));
    return lds_depth;
}
// tray_scene_set_wavefront asks for another pool size: the buffers go (drop_pool), the next render call allocates them anew
inline bool wish_changed(const State& b, uint32_t n_tiles, uint32_t req_before, uint32_t req_after) {
    return b.pool && slot_wish(n_tiles, req_after) != slot_wish(n_tiles, req_before);
}

// ---- procedures

// A device whose free memory cannot be asked counts as 16 GiB free where a pool or a cache budget is sized (here), as nothing free where cache_ensure
// weighs a cache for a pool that is there, and as roomy where table_ensure applies the third-of-free rule
template <class Ops>
inline uint64_t free_or_16g(Ops& ops) {
    uint64_t free_b = 0;
    return ops.free_bytes(&free_b) ? free_b : (uint64_t)16 << 30;
}
// the parts of `what` that exist go (the caller has made sure that no launch still reads them); the cache's lanes stay: before a wavefront cache is
// allocated anew they are its budget
template <class Ops>
inline void drop(Ops& ops, State& b, unsigned what) {
    what &= (b.pool ? kPool : 0u) | (b.cache ? kCache : 0u) | (b.table ? kTable : 0u);
    if (what) ops.drop(what);
    if (what & kPool) { b.pool = false; b.pool_slots = b.pool_stack_bytes = b.pool_quad_stack_words = 0u; b.pool_animated = false; }
    if (what & kCache) { b.cache = false; b.cache_bytes = 0; }
    if (what & kTable) { b.table = false; b.table_cap = b.table_stride = 0u; b.table_built = false; }
}
template <class Ops>
inline void drop_pool(Ops& ops, State& b) { drop(ops, b, kPool); b.wf_shrunk = false; }

template <class Ops>
inline int cache_grant(Ops& ops, State& b, const Facts& f, uint32_t lanes) {
    const uint64_t bytes = cache_bytes(f.n_moving, f.wavefront, lanes);
    if (!ops.grant_cache(lanes, bytes)) return TRAY_E_NOMEM;
    b.cache = true; b.cache_lanes = lanes; b.cache_bytes = bytes;
    return TRAY_OK;
}

// Fits the launch buffers a frame update handed on (none for a new scene) to the frame of `f`: the cache keeps its lanes if it was made for this schedule
// (the tile kernel's: for as many resident threads), else they are budgeted anew; the pool stays if it was made for these stacks and kernels and is no
// larger than the cache's lanes or the wish (a pool that memory made smaller stays), or was sized for table launches and the table came along. A kept pool
// serves as it is (launch_wavefront re-initialises chunk records and control words, the bins are zero between tiles). Returns whether the pool was kept.
template <class Ops>
inline bool fit(Ops& ops, State& b, const Facts& f) {
    const bool moving = f.animated && f.n_moving > 0;
    // (what the previous frame held counts as free, or the budget -- and with it the pool size -- would depend on which frame came first)
    const uint64_t reclaimable = b.cache_bytes + (b.pool ? pool_bytes(b.pool_slots) : 0u);
    const bool keep_lanes = moving && b.cache_lanes != 0u && b.wavefront == f.wavefront && (f.wavefront || b.cache_lanes == f.tile_workgroups * TR_BLOCK);
    const uint32_t lanes = !moving ? 0u : keep_lanes ? b.cache_lanes : f.wavefront ? cache_budget(f.n_tiles, f.n_moving, free_or_16g(ops) + reclaimable) : f.tile_workgroups * TR_BLOCK;
    if (!keep_lanes || b.cache_bytes < cache_bytes(f.n_moving, f.wavefront, lanes)) drop(ops, b, kCache);   // (every path fills its columns before it reads them)
    b.cache_lanes = lanes;
    const bool keep_pool = b.pool && f.wavefront && b.pool_stack_bytes == f.stack_bytes && b.pool_quad_stack_words == f.quad_stack_words &&
                           b.pool_animated == f.animated && (b.pool_slots <= (lanes ? lanes : slot_wish(f.n_tiles, f.req_slots)) || (b.last_used_table && b.table));
    if (!keep_pool) drop_pool(ops, b);
    b.wavefront = f.wavefront;
    b.table_stride = 0u; b.table_built = false; b.last_used_table = false;   // (the table is built anew by the frame's first launch that wants it)
    return keep_pool;
}
// A frame update (or a new scene): fit, then the tile kernel's cache -- the wavefront schedule's is allocated by the first launch that evaluates per
// path (prepare). *pool_kept: what fit returned.
template <class Ops>
inline int frame(Ops& ops, State& b, const Facts& f, bool* pool_kept) {
    *pool_kept = fit(ops, b, f);
    if (f.n_moving && !f.wavefront && !b.cache && cache_grant(ops, b, f, b.cache_lanes) != TRAY_OK) return TRAY_E_NOMEM;
    return TRAY_OK;
}

// The wavefront schedule's per-path cache, with a record for every pool slot: the budgeted lanes or the pool's slots. A pool larger than the budget (sized
// for table launches) stays if a cache for all of it fits in two fifths of the free memory, else it goes and is sized anew for the cache; a cache too
// small for the pool is allocated anew. Halved while the allocation is refused, never below the pool's slots or 64 chunks.
template <class Ops>
inline int cache_ensure(Ops& ops, State& b, const Facts& f) {
    if (!f.wavefront || f.n_moving == 0u) return TRAY_OK;
    if (b.pool && b.pool_slots > b.cache_lanes) {
        uint64_t free_b = 0;
        if (!ops.free_bytes(&free_b)) free_b = 0;
        if (cache_bytes(f.n_moving, f.wavefront, b.pool_slots) > free_b / 5u * 2u) {
            if (const int rc = ops.synchronise()) return rc;
            drop(ops, b, kPool);
        }
    }
    if (b.cache && (!b.pool || b.pool_slots <= b.cache_lanes)) return TRAY_OK;
    if (b.cache) {
        if (const int rc = ops.synchronise()) return rc;
        drop(ops, b, kCache);
    }
    const uint32_t pool_slots = b.pool ? b.pool_slots : 0u, floor_lanes = b.pool ? pool_slots : kMinSlots;
    for (uint32_t lanes = std::max(b.cache_lanes, pool_slots);; lanes = std::max(floor_lanes, lanes / 2u / TR_BLOCK * TR_BLOCK)) {
        const int rc = cache_grant(ops, b, f, lanes);
        if (rc == TRAY_OK || lanes <= floor_lanes) return rc;
    }
}
// The transform table of a moving scene's frame with `stride` records per time index, built once per frame on the launch's stream by the first launch
// that reads it; TRAY_E_NOMEM if the buffer cannot be had
template <class Ops>
inline int table_ensure(Ops& ops, State& b, const Facts& f, uint32_t stride) {
    if (b.table && b.table_cap < stride) drop(ops, b, kTable);   // (the buffer handed on from the previous frame is too small for this frame's records)
    if (b.table && b.table_stride != stride) { b.table_stride = stride; b.table_built = false; }
    if (!b.table) {
        // room for what any frame of the sequence can move (instances whose transforms have several keyframes), if that much is to be had
        uint32_t cap = std::max(stride, f.xf_movable);
        // by the library's own rule (nobody asked for the table) it takes at most a third of what is free: on a device shared with other
        // allocators 22.5 GB for eleven movers must not be what starves them
        const bool own_rule = f.table_req < 0 && !getenv("TRAYHIP_XF_TABLE");
        for (;;) {   // (the sequence's headroom first, then this frame's records alone)
            const uint64_t bytes = table_bytes(cap);
            uint64_t free_b = 0;
            const bool room = !own_rule || !ops.free_bytes(&free_b) || bytes <= free_b / 3u;
            if (room && ops.grant_table(bytes)) break;
            if (cap == stride) return TRAY_E_NOMEM;
            cap = stride;
        }
        b.table = true; b.table_stride = stride; b.table_cap = cap; b.table_built = false;
    }
    if (!b.table_built) {
        if (const int rc = ops.table_build(stride)) return rc;
        b.table_built = true;
        return TRAY_OK;
    }
    return ops.table_wait();
}

// What a render call of `samples` camera samples needs of the launch buffers: 1. table or per-path evaluation (table_wanted); 2. the chosen one exists,
// else the other serves (the table is smaller from a few million slots on); 3. the pool, kept or as large as the cache's lanes or the memory rule grant,
// halved while the allocation is refused (fragmentation, another scene's pool) down to 64 chunks, then TRAY_E_NOMEM with the handle as it was (ADVICE
// round 4); 4. a launch that reads the cache has a record for every slot. b.last_used_table: which of cache or table the launch reads.
template <class Ops>
inline int prepare(Ops& ops, State& b, const Facts& f, uint64_t samples) {
    b.last_used_table = false;
    const uint32_t stride = f.n_moving + (f.camera_animated ? 1u : 0u);
    bool table = false;
    if (f.animated && stride != 0u) {
        int rc = table_wanted(f.table_req, samples, b) ? TRAY_E_NOMEM : cache_ensure(ops, b, f);
        if (rc == TRAY_E_NOMEM) {   // (the table wanted, or no room for the cache)
            rc = table_ensure(ops, b, f, stride);
            table = rc == TRAY_OK;
            if (rc == TRAY_E_NOMEM) rc = cache_ensure(ops, b, f);
        }
        if (rc != TRAY_OK) return rc;
    }
    b.last_used_table = table;
    const bool reads_cache = f.wavefront && !table && f.n_moving != 0u;   // (the tile kernel's cache has a column per resident thread: fit)
    if (const int rc = ops.refusal()) return rc;
    if (f.wavefront && !b.pool) {
        // (a launch that reads no per-path cache -- a static scene, or the frame's table instead: ADVICE round 5 -- is bounded by the pool's own bytes alone)
        uint32_t n_slots = reads_cache ? std::min(b.cache_lanes, slot_wish(f.n_tiles, f.req_slots))
                                       : slot_fit(f.n_tiles, slot_wish(f.n_tiles, f.req_slots), free_or_16g(ops), f.req_slots);
        for (;;) {
            const int rc = ops.grant_pool(n_slots);
            if (rc == TRAY_OK) break;
            if (rc != TRAY_E_NOMEM) return rc;
            if (n_slots / 2u < kMinSlots) { ops.no_pool(n_slots); return TRAY_E_NOMEM; }
            n_slots = n_slots / 2u / TR_BLOCK * TR_BLOCK;
            b.wf_shrunk = true;
        }
        b.pool = true; b.pool_slots = n_slots;
        b.pool_stack_bytes = f.stack_bytes; b.pool_quad_stack_words = f.quad_stack_words; b.pool_animated = f.animated;
    }
    // the stage kernels index the per-path cache by pool slot: it must have a record for every slot
    if (reads_cache && (!b.cache || b.pool_slots > b.cache_lanes)) { ops.cache_short(b.pool_slots, b.cache ? b.cache_lanes : 0u); return TRAY_E_DEVICE; }
    return TRAY_OK;
}

}  // namespace tr_lbplan
