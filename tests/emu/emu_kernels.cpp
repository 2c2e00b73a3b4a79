// TEST INFRASTRUCTURE ONLY: the device source of libtrayhip.so compiled for the host (hip_emu.h) and driven one thread at a
// time. Entry points mirror what the library does around the same kernels (scene upload, pool fields, queues, launch geometry).
#include "hip_emu.h"
#include <sys/mman.h>   // (the sparse transform table of emu_render_tiles)
#ifdef TR_COOP_HIST   // tools/coop_histogram.py: [rays staged][lanes that asked] of every cooperative small-mesh test (dev_geom.h: mesh_leaf_coop)
namespace tr { unsigned long long tr_coop_hist[65 * 65]; }
extern "C" unsigned long long* emu_coop_hist(void) { return tr::tr_coop_hist; }
#endif

#ifdef TR_EMU_PROFILE   // divergence profile: see hip_emu.h; block barriers are ignored (they separate tiles, not stages)
#include <dlfcn.h>
#include <map>
#include <unordered_map>
#define NOINSTR __attribute__((no_instrument_function))
namespace hip_emu {
struct ProfAgg { uint64_t lane_calls = 0, wave_calls = 0, lanes = 0, segments = 0; };
struct ProfState {
    std::unordered_map<void*, uint32_t> lane;                 // calls of the running lane in its current segment
    std::unordered_map<void*, std::pair<uint32_t, uint64_t>> wave[MAX_THREADS / WAVE];   // fn -> (max over lanes, sum over lanes) in the wave's segment
    std::unordered_map<void*, uint32_t> wave_lanes[MAX_THREADS / WAVE];
    std::unordered_map<void*, ProfAgg> total;
    bool on = false;
};
static ProfState g_prof;
NOINSTR inline ProfState& prof() { return g_prof; }
NOINSTR void prof_lane_done(uint32_t wave) {
    ProfState& p = prof();
    if (!p.on) return;
    for (auto& kv : p.lane) {
        auto& w = p.wave[wave][kv.first];
        w.first = std::max(w.first, kv.second); w.second += kv.second;
        p.wave_lanes[wave][kv.first] += 1;
    }
    p.lane.clear();
}
NOINSTR void prof_wave_done(uint32_t wave) {
    ProfState& p = prof();
    if (!p.on) return;
    for (auto& kv : p.wave[wave]) {
        ProfAgg& a = p.total[kv.first];
        a.wave_calls += kv.second.first; a.lane_calls += kv.second.second; a.lanes += p.wave_lanes[wave][kv.first]; a.segments += 1;
    }
    p.wave[wave].clear(); p.wave_lanes[wave].clear();
}
}  // namespace hip_emu
extern "C" {
NOINSTR void __cyg_profile_func_enter(void* fn, void*) { hip_emu::ProfState& p = hip_emu::prof(); if (p.on && hip_emu::block().simt) ++p.lane[reinterpret_cast<void*>((reinterpret_cast<uintptr_t>(fn) << 3) | (hip_emu::prof_phase_of[hip_emu::block().current & 1023u] & 7u))]; }
NOINSTR void __cyg_profile_func_exit(void*, void*) {}
NOINSTR void emu_profile_start(void) { hip_emu::ProfState& p = hip_emu::prof(); p.total.clear(); p.on = true; }
// writes "lane_calls wave_calls lanes segments symbol" lines; returns the number of functions
NOINSTR int emu_profile_dump(const char* path) {
    hip_emu::ProfState& p = hip_emu::prof();
    p.on = false;
    FILE* f = std::fopen(path, "w");
    if (!f) return -1;
    std::unordered_map<void*, hip_emu::ProfAgg> by_fn;   // the phases of a function, added up
    for (auto& kv : p.total) {
        hip_emu::ProfAgg& a = by_fn[reinterpret_cast<void*>(reinterpret_cast<uintptr_t>(kv.first) >> 3)];
        a.lane_calls += kv.second.lane_calls; a.wave_calls += kv.second.wave_calls; a.lanes += kv.second.lanes; a.segments += kv.second.segments;
    }
    for (auto& kv : by_fn) {
        Dl_info info;
        const char* name = (dladdr(kv.first, &info) && info.dli_sname) ? info.dli_sname : "?";
        std::fprintf(f, "%llu %llu %llu %llu %s\n", (unsigned long long)kv.second.lane_calls, (unsigned long long)kv.second.wave_calls,
                     (unsigned long long)kv.second.lanes, (unsigned long long)kv.second.segments, name);
    }
    if (std::getenv("TR_PROFILE_PHASES"))   // the same rows per phase (TR_EMU_PHASE: the query passes LIGHT = 1, MIS = 2, PATH = 3; 0 = everything else), name suffixed "@phase"
        for (auto& kv : p.total) {
            Dl_info info;
            void* fn = reinterpret_cast<void*>(reinterpret_cast<uintptr_t>(kv.first) >> 3);
            const char* name = (dladdr(fn, &info) && info.dli_sname) ? info.dli_sname : "?";
            std::fprintf(f, "%llu %llu %llu %llu %s@%u\n", (unsigned long long)kv.second.lane_calls, (unsigned long long)kv.second.wave_calls,
                         (unsigned long long)kv.second.lanes, (unsigned long long)kv.second.segments, name, (unsigned)(reinterpret_cast<uintptr_t>(kv.first) & 7u));
        }
    std::fclose(f);
    return (int)by_fn.size();
}
}
#endif

#include "../../tray_rust_amd/csrc/hip/kernels.hip"
#include "../../tray_rust_amd/csrc/hip/kernel_select.h"   // the library's choice of the instantiation ...
#include "../../tray_rust_amd/csrc/hip/launch_rules.h"    // ... its launch rules ...
#include "../../tray_rust_amd/csrc/hip/scene_plan.h"      // ... its per-scene decisions ...
#include "../../tray_rust_amd/csrc/hip/wavefront_plan.h"  // ... and its wavefront schedule: the emulation applies them, it has no copy
#include "wavefront_plan_record.h"                        // (tests/test_wavefront_plan.py's exports)
#include "../../tray_rust_amd/csrc/hip/launch_buffers_plan.h"   // the library's launch-buffer plan, which the emulation does not run: its own buffers are vectors
#include "launch_buffers_plan_record.h"                   // (tests/test_launch_buffers_plan.py's exports)
#ifdef TR_SAMPLE_RANGES   // (emu_sample_ranges.cpp) the kernels take a sample range: EMU_RANGE appends it to a call, and only there do the two builds differ
#define EMU_RANGE(...) , __VA_ARGS__
#else
#define EMU_RANGE(...)
#endif

namespace trayh { void set_error(const std::string&) {} }

namespace {

uint32_t g_retraced = 0;   // accumulated over the calls of this process; read and reset by emu_retraced()
uint32_t g_wf_deferred = 0;   // rays k_wf_trace_dyn handed to k_wf_trace_fallback; read and reset by emu_wf_deferred()

struct EmuScene {
    DevScene d{};
    std::vector<DevMaterial> mats;
    std::vector<tray::FlatLeaf> flat_leaves;
    std::vector<tray::FlatInst> flat_insts;
    std::vector<uint8_t> tri_leaf;
    tray::PairedTrees paired;   // the trees in device order, as tray_scene_create uploads them
    tray::QuadTrees quads;      // ... and as the wavefront traversal's 128-byte records
    std::vector<tray::QuadNode> all_quads;
    std::vector<tray::WfInst> wf_insts;
    std::vector<uint8_t> perm_pool;
    uint32_t retraced = 0;   // rays the flat loop handed to trace_bvh
    tr_plan::ScenePlan plan;   // the library's decisions for the scene (scene_plan.h); the LDS layout by lds_layout()
    uint32_t quad_words = 0;   // stack words per lane of the wavefront traversal (node entries are two words, up to three per record)
};

void make_scene(const TrayFlatScene* f, EmuScene& e) {
    DevScene& d = e.d;
    if (!tray::pair_trees(f, e.paired)) throw std::runtime_error("BVH arrays do not describe trees");
    d.instances = f->instances; d.top_nodes = e.paired.top.data(); d.top_order = f->top_order; d.meshes = e.paired.meshes.data();
    d.mesh_nodes = e.paired.mesh.data(); d.tri_verts = f->tri_verts; d.tri_attrs = f->tri_attrs;
    tray::quad_trees(f, e.quads);
    e.all_quads = e.quads.mesh;   // one buffer, as tray_scene_create uploads it: the BVH<Triangle>s, then BVH<Instance>
    e.all_quads.insert(e.all_quads.end(), e.quads.top.begin(), e.quads.top.end());
    d.quads = reinterpret_cast<const float4*>(e.all_quads.data()); d.top_quad_first = (uint32_t)e.quads.mesh.size();
    tray::wf_inst_records(f, e.quads.mesh_first, e.wf_insts);
    d.wf_insts = e.wf_insts.data();
    e.mats.resize(f->n_materials);
    for (uint32_t i = 0; i < f->n_materials; ++i) e.mats[i] = lower_material(f->materials[i], f->merl_tables);
    d.materials = e.mats.data(); d.merl_data = f->merl_data; d.lights = f->lights;
    d.textures = f->n_textures ? f->textures : nullptr; d.tex_frames = f->tex_frames; d.tex_data = f->tex_data;
    d.filter_table = f->film.table; d.filter_x = f->film.table_x; d.filter_y = f->film.table_y;
    d.xf_levels = f->xf_levels; d.keyframes = f->keyframes; d.knots = f->knots; d.color_keys = f->color_keys;
    d.xf_cache = nullptr; d.moving_ids = nullptr; d.n_moving = 0; d.xf_cache_lanes = 0; d.xf_aos = 0; d.xf_table = 0; d.xf_stride = 0; d.xf_tab = nullptr; d.xf_tab_stride = 0; d.pad_tab = 0;
    d.n_instances = f->n_instances; d.n_lights = f->n_lights; d.min_depth = f->min_depth; d.max_depth = f->max_depth;
    d.width = f->film.width; d.height = f->film.height; d.frame = f->frame; d.film_rows = 0; d.coop_offset = 0; d.integrator = f->integrator;
    d.filter_w = f->film.filter_w; d.filter_h = f->film.filter_h; d.inv_w = f->film.inv_w; d.inv_h = f->film.inv_h;
    d.fpw = f->film.filter_pixel_w; d.fph = f->film.filter_pixel_h;
    d.camera_p = &f->camera;
    e.perm_pool.resize(TR_PERM_BYTES);
    perm_pool_build(f->max_depth + 1u, e.perm_pool.data());
    d.perm_pool = e.perm_pool.data();
    tray::flat_loop_gates(f, e.paired, TR_COOP_MAX_TRIS, e.flat_leaves, e.flat_insts, e.tri_leaf);
    d.flat_leaves = e.flat_leaves.data(); d.flat_insts = e.flat_insts.data(); d.n_flat_leaves = (uint32_t)e.flat_leaves.size(); d.tri_leaf = e.tri_leaf.data();
    d.retraced = &g_retraced;
    d.mesh_keys = f->mesh_keys; d.key_times = f->key_times;
    e.quad_words = 2u * (e.quads.top_pend + e.quads.mesh_pend) + 34u;
    tr_plan::ScenePlan& p = e.plan;
    tr_plan::plan_motion(f, p);
    tr_plan::plan_materials(e.mats, p);
    tr_plan::plan_light_filter(f, p);
    p.film_rows_ok = tr_plan::film_rows_ok(f->film);
    p.wavefront = tr_plan::wavefront(f, e.paired.narrow && e.quads.narrow && e.quads.ordered, p);
    tr_plan::plan_stacks(f, tr_plan::mesh_depths(f), p);
}

// the dynamic LDS of the kernels that traverse; coop / film_rows: 0 = without the cooperative small-mesh test / the row-binned film
void lds_layout(const TrayFlatScene* f, EmuScene& e, bool coop, bool film_rows) {
    e.d.film_rows = (film_rows && e.plan.film_rows_ok) ? 1u : 0u;
    tr_plan::plan_lds(f, coop, e.d.film_rows != 0u, e.plan);
    e.d.coop_offset = e.plan.coop_offset; e.d.win_offset = e.plan.win_offset;
}

using hip_emu::launch;
using hip_emu::launch_simt;
using tr_wfplan::QA; using tr_wfplan::QB; using tr_wfplan::QC; using tr_wfplan::QR; using tr_wfplan::Queue;

// The wavefront schedule's Ops (wavefront_plan.h: round) of the emulation: the plan's launch groups as SIMT emulations over ONE view of the pool. After a
// failed launch_simt nothing more is launched (rc). The traversal grid is the caller's, the fallback kernel runs as one workgroup.
struct EmuWfOps {
    const DevScene& d;
    WfPool pool;
    tr_wfplan::Buffers b;
    WfChunk* chunks;
    float* bins;
    const uint2* tiles;
    uint32_t n_items, tile_count, spp, kf;
    float* rgbw;
    uint32_t* counters;
    DevStats* stats;
    uint32_t slice_shift, smp_begin, smp_end;
    uint32_t n_chunks, trace_blocks, lds_depth;
    size_t fb_lds, bin_ctl_words;
    WfBinGrid bin_grid;
    int rc = 0;

    template <class F> void k(uint32_t blocks, F&& f, size_t lds = 0) { if (rc == 0) rc = launch_simt(blocks, TR_BLOCK, f, lds); }
    uint32_t q_blocks() const { return (n_chunks + WF_SEGS - 1u) / WF_SEGS * WF_SEGS; }   // grid of the one-thread-per-entry kernels
    uint32_t bin_blocks() const { return (pool.seg_cap + WF_BIN_EPB - 1u) / WF_BIN_EPB * WF_SEGS; }
    uint32_t n_active() const { return n_chunks * TR_BLOCK; }
    uint32_t* qc(bool stage_c) const { return stage_c ? b.q[QC] : nullptr; }

    template <int A> void advance() {
        k(n_chunks, [&] { k_wf_advance<A>(d, pool, chunks, bins, tiles, n_items, tile_count, 1u, spp, kf, rgbw, counters, counters + 1, stats,
                                          b.q[QA], b.q[QR], b.qctl, slice_shift EMU_RANGE(smp_begin, smp_end)); });
    }
    template <int A> void regen() {
        k(q_blocks(), [&] { k_wf_regen<A>(d, pool, chunks, tiles, tile_count, 1u, spp, kf, stats, b.q[QR], b.q[QA], b.qctl, slice_shift); });
    }
    template <int S> void bin(Queue from, Queue to) {
        uint32_t* const ctl = b.bin_ctl + (size_t)S * 2u * WF_SEGS * WF_BINS;
        k(bin_blocks(), [&] { k_wf_bin_hist<S>(pool, b.q[from], b.qctl, ctl, bin_grid); });
        k(bin_blocks(), [&] { k_wf_bin_scatter<S>(pool, b.q[from], b.q[to], b.qctl, ctl, bin_grid); });
    }
    template <int S, int A> void trace(Queue from, Queue fallback, uint32_t fused) {
        k(trace_blocks, [&] { k_wf_trace_dyn<S, A>(d, pool, b.q[from], b.qctl, stats, lds_depth, b.overflow, b.q[fallback], fused); }, (size_t)lds_depth * TR_BLOCK * 4);
        k(1u, [&] { k_wf_trace_fallback<S, A>(d, pool, b.qctl, b.q[fallback], fused); }, fb_lds);
        g_wf_deferred += b.qctl[WF_FB_WORD + S];
    }
    int clear_qctl() { std::memset(b.qctl, 0, WF_QCTL_WORDS * sizeof(uint32_t)); return 0; }
    int clear_bin_ctl() { std::memset(b.bin_ctl, 0, bin_ctl_words * sizeof(uint32_t)); return 0; }
    void sort() { k(n_chunks, [&] { k_wf_sort<0>(d, pool, n_active(), b.qctl, b.kq); }); }
    template <int A, int K> void shade_kind() { k(q_blocks(), [&] { k_wf_shade_kind<A, K>(d, pool, b.kq, b.qctl, stats, b.q[QA], b.q[QB]); }); }
    template <int A> void begin() { k(n_chunks, [&] { k_wf_begin<A>(d, pool, n_active(), stats, b.q[QB], b.qctl, b.kq); }); }
    template <int A, int K> void query_kind(bool stage_c) { k(q_blocks(), [&] { k_wf_query_kind<A, K>(d, pool, b.kq, qc(stage_c), b.qctl, stats, b.q[QA]); }); }
    template <int A> void query(bool stage_c) { k(n_chunks, [&] { k_wf_query<A, FEAT_ALL | FEAT_TEX>(d, pool, n_active(), qc(stage_c), b.qctl, stats, b.q[QA]); }); }
};

}  // namespace

extern "C" {

// k_debug_intersect on n rays (what tray_debug_intersect launches)
int emu_debug_intersect(const TrayFlatScene* f, uint32_t n, const TrayRay* rays, TrayHit* hits) {
    EmuScene e;
    make_scene(f, e);
    const int anim = e.plan.anim_debug();
    if (anim == 3) launch((n + TR_BLOCK - 1) / TR_BLOCK, TR_BLOCK, [&] { k_debug_intersect<3>(e.d, n, rays, hits); });
    else if (anim == 2) launch((n + TR_BLOCK - 1) / TR_BLOCK, TR_BLOCK, [&] { k_debug_intersect<2>(e.d, n, rays, hits); });
    else launch((n + TR_BLOCK - 1) / TR_BLOCK, TR_BLOCK, [&] { k_debug_intersect<0>(e.d, n, rays, hits); });
    return 0;
}

// k_debug_sample_radiance<0 | 2> for n (pixel, sample) items (what tray_debug_sample_radiance launches; ANIM = 2 evaluates the
// spline stacks at every use, as the library does for its debug kernels on moving scenes)
int emu_debug_sample_radiance(const TrayFlatScene* f, uint32_t n, const uint32_t* px, const uint32_t* py, const uint32_t* si, uint32_t spp,
                              uint64_t seed, float* out) {
    EmuScene e;
    make_scene(f, e);
    const uint32_t kf = tr_rules::frame_key(seed, e.d.frame);
    const int anim = e.plan.anim_debug();
    if (anim == 3) launch((n + TR_BLOCK - 1) / TR_BLOCK, TR_BLOCK, [&] { k_debug_sample_radiance<3>(e.d, n, px, py, si, spp, kf, out); });
    else if (anim == 2) launch((n + TR_BLOCK - 1) / TR_BLOCK, TR_BLOCK, [&] { k_debug_sample_radiance<2>(e.d, n, px, py, si, spp, kf, out); });
    else launch((n + TR_BLOCK - 1) / TR_BLOCK, TR_BLOCK, [&] { k_debug_sample_radiance<0>(e.d, n, px, py, si, spp, kf, out); });
    return 0;
}

// launch_sampler (device_api.hip) for the tiles given: thread_work with sampler::Uniform / sampler::Adaptive, or LowDiscrepancy (min_spp = the render's
// spp) over the samples [smp_begin, smp_end) of the frame, 0 / 0 = all of them. batch_tiles bounds the tiles per batch (0 = all at once), so that tests
// can see batches add up. stats_out: samples, vertices, rays.
static int render_sampler(const TrayFlatScene* f, const uint32_t* tiles_xy, uint32_t tile_count, uint32_t kind, uint32_t min_spp, uint32_t max_spp,
                          uint32_t smp_begin, uint32_t smp_end, uint64_t seed, float* rgbw, uint32_t batch_tiles, unsigned long long* stats_out) {
    EmuScene e;
    make_scene(f, e);
    const uint32_t kf = tr_rules::frame_key(seed, e.d.frame);
    std::vector<uint2> tiles(tile_count);
    for (uint32_t i = 0; i < tile_count; ++i) tiles[i] = make_uint2(tiles_xy[2 * i], tiles_xy[2 * i + 1]);
    DevStats stats;
    std::memset(&stats, 0, sizeof stats);
    if (kind > TRAY_SAMPLER_ADAPTIVE) return -1;
    SamplerPass sp{};
    sp.kind = kind; sp.min_spp = tr_rules::round_spp(min_spp); sp.max_spp = tr_rules::round_spp(max_spp);   // (tray_scene_set_sampler)
    if (kind == TRAY_SAMPLER_ADAPTIVE && sp.max_spp < sp.min_spp) return -1;
    tr_rules::whole_frame_range(min_spp, smp_begin, smp_end);
    const uint32_t rounds = tr_rules::sampler_plan(sp, sp.min_spp);
    const uint32_t batch = batch_tiles ? std::min(batch_tiles, std::max(tile_count, 1u)) : std::max(tile_count, 1u);
    std::vector<uint32_t> px_state((size_t)batch * 64u);
    std::vector<float> px_avg((size_t)batch * 64u), px_lum((size_t)batch * 64u * std::max(sp.lum_cap, 1u));
    const uint32_t chunk = tr_rules::whole_queue(tile_count).chunk;
    int rc = 0;   // (the window is shared by the block's threads: a SIMT emulation, as for k_path_tiles)
    for (uint32_t item0 = 0; item0 < tile_count; item0 += batch) {
        const uint32_t n_items = std::min(batch, tile_count - item0), n_px = n_items * 64u;
        std::fill(px_state.begin(), px_state.end(), 0u); std::fill(px_avg.begin(), px_avg.end(), 0.0f);
        for (uint32_t j = 0; j < rounds; ++j) {
            tr_rules::sampler_round(sp, j, smp_end ? smp_end - smp_begin : 0u);
            const uint32_t group = tr_rules::sampler_group(sp.count, SP_GROUP_MAX);
            const uint32_t grid = (n_items + group - 1u) / group;
            select_sampler_pass(e.plan.anim_debug(), sampler_lean(e.plan.feat, f->integrator), [&](auto kernel) {
                rc = launch_simt(grid, TR_BLOCK, [&] { kernel(e.d, tiles.data(), item0, n_items, chunk, 1u, kf, sp, px_state.data(), px_lum.data(), rgbw, &stats, group EMU_RANGE(smp_begin)); });
            });
            if (rc != 0) return -3;
            if (kind == TRAY_SAMPLER_ADAPTIVE)
                launch((n_px + TR_BLOCK - 1) / TR_BLOCK, TR_BLOCK, [&] { k_sampler_decide(n_px, sp, px_state.data(), px_avg.data(), px_lum.data()); });
        }
    }
    if (stats_out) { stats_out[0] = stats.samples; stats_out[1] = stats.vertices; stats_out[2] = stats.rays; }
    return 0;
}
int emu_render_sampler(const TrayFlatScene* f, const uint32_t* tiles_xy, uint32_t tile_count, uint32_t kind, uint32_t min_spp, uint32_t max_spp,
                       uint64_t seed, float* rgbw, uint32_t batch_tiles, unsigned long long* stats_out) {
    return render_sampler(f, tiles_xy, tile_count, kind, min_spp, max_spp, 0u, 0u, seed, rgbw, batch_tiles, stats_out);
}

// Debugging aid: the loop of k_debug_sample_radiance<0> for ONE sample with the lane state printed after every vertex
int emu_trace_sample(const TrayFlatScene* f, uint32_t px, uint32_t py, uint32_t si, uint32_t spp, uint64_t seed) {
    EmuScene e;
    make_scene(f, e);
    const uint32_t kf = tr_rules::frame_key(seed, e.d.frame);
    hip_emu::launch(1, 1, [&] {
        const DevScene& sc = e.d;
        TR_DYN_LDS(uint32_t, s_stack);
        Counters cnt; cnt.rays = 0; cnt.vertices = 0;
        const uint32_t kp = key_pixel(kf, py * sc.width + px);
        float sx, sy, t;
        pixel_sample(kp, si, spp, px, py, sx, sy, t);
        Lane ln;
        lane_start_sample(ln, camera_ray<0>(sc, sx, sy, t), key_sample(kp, si));
        while (ln.flags & LF_ALIVE) {
            for (int stage = 0; stage < 3; ++stage) {
                const bool alive = (ln.flags & LF_ALIVE) != 0u;
                const bool want_ray = alive && (stage == 0 || (stage == 1 && (ln.flags & LF_SHADOW)) || (stage == 2 && (ln.flags & LF_MIS)));
                TraceResult tr_; tr_.hit = false; tr_.rec.t = 0.0f; tr_.rec.inst = 0xffffffffu; tr_.rec.prim = 0u; tr_.rec.b1 = 0.0f; tr_.rec.b2 = 0.0f;
                if (want_ray) { const Ray r = stage == 0 ? stage_a_ray(ln) : (stage == 1 ? stage_b_ray(ln) : stage_c_ray(ln)); tr_ = trace<0>(&e.d, s_stack, r, stage == 1, want_ray); }
                if (!alive) continue;
                if (stage == 0) { if (tr_.hit) vertex_begin<0>(sc, ln, tr_.rec, cnt); else ln.flags &= ~LF_ALIVE; if (tr_.hit) std::fprintf(stderr, "device  bounce %u inst %u", ln.bounce, tr_.rec.inst); }
                else if (stage == 1) {
                    std::fprintf(stderr, "\ndevice    light sample: pdf %.9g li %.9g %.9g %.9g shadow-ray %d occluded %d w_i %.9g %.9g %.9g\n", ln.pdf_l, ln.li.x, ln.li.y, ln.li.z,
                                 (int)((ln.flags & LF_SHADOW) != 0), (int)tr_.hit, ln.wi_l.x, ln.wi_l.y, ln.wi_l.z);
                    vertex_queries<0, FEAT_ALL>(sc, ln, tr_.hit);
                    std::fprintf(stderr, "device    after queries: direct %.9g %.9g %.9g mis %d (cos, w, pdf) %.9g %.9g %.9g f %.9g %.9g %.9g\n", ln.direct.x, ln.direct.y, ln.direct.z,
                                 (int)((ln.flags & LF_MIS) != 0), ln.li.x, ln.li.y, ln.li.z, ln.mis_f.x, ln.mis_f.y, ln.mis_f.z);
                }
                else {
                    const f3 tv = ln.t_vertex;
                    const uint32_t b = ln.bounce;
                    const bool cont = vertex_end<0>(sc, ln, tr_.hit, tr_.rec);
                    std::fprintf(stderr, " li %.9g %.9g %.9g  throughput %.9g %.9g %.9g  illum %.9g %.9g %.9g\n", ln.direct.x, ln.direct.y, ln.direct.z, tv.x, tv.y, tv.z,
                                 ln.illum.x, ln.illum.y, ln.illum.z);
                    (void)b;
                    if (!cont) ln.flags &= ~LF_ALIVE;
                }
            }
        }
    });
    return 0;
}

// k_debug_bsdf: BSDF::eval / pdf / sample of one material on the canonical frame (what tray_debug_bsdf launches)
int emu_debug_bsdf(const TrayFlatScene* f, uint32_t material_id, uint32_t flags, uint32_t n, const float* dirs, const float* u3, float* out) {
    if (material_id >= f->n_materials) return -1;
    EmuScene e;
    make_scene(f, e);
    TrayInstance fake;
    std::memset(&fake, 0, sizeof fake);
    fake.material_id = material_id;
    e.d.instances = &fake;
    launch((n + 63) / 64, 64, [&] { k_debug_bsdf(e.d, flags, n, dirs, u3, out); });
    return 0;
}

// One stage of the wavefront traversal over n rays, through the pool fields and the queue the stage kernels use:
//   k_wf_trace_dyn; stage 0 = A (closest hit from
//   F_O / F_D), 1 = B (any hit on the segment F_P + t F_AUX, t in (0.001, 0.999)), 2 = C (closest hit from F_P along F_AUX).
// lds_depth < full depth exercises the HBM overflow part of the stacks. Output per ray: hit flag, t, inst, prim, b1, b2.
int emu_wf_trace(const TrayFlatScene* f, int stage, uint32_t n, const TrayRay* rays, uint32_t lds_depth, uint32_t blocks,
                 uint32_t* hit, float* t, uint32_t* inst, uint32_t* prim, float* b1, float* b2) {
    EmuScene e;
    make_scene(f, e);
    const uint32_t n_slots = (n + TR_BLOCK - 1) / TR_BLOCK * TR_BLOCK;
    std::vector<float> pool_data((size_t)F_COUNT * n_slots, 0.0f);
    WfPool pool{pool_data.data(), n_slots, wf_seg_cap(n_slots / TR_BLOCK)};
    std::vector<uint32_t> queue((size_t)WF_SEGS * pool.seg_cap * WF_RAY_WORDS), qctl(WF_QCTL_WORDS, 0u);
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t s = n - 1u - i;   // any order inside a segment: slots keep their place, only indices travel
        const uint32_t seg = (s / TR_BLOCK) & (WF_SEGS - 1u);   // the segment of the slot's chunk (wavefront.h)
        const f3 o = mk(rays[s].o[0], rays[s].o[1], rays[s].o[2]), dd = mk(rays[s].d[0], rays[s].d[1], rays[s].d[2]);
        wf_put_ray(queue.data(), (size_t)seg * pool.seg_cap + qctl[seg * WF_SEG_STRIDE + stage]++, s, o, dd,
                   LF_ALIVE | (stage == 0 && rays[s].min_t == 0.0f ? WF_CAMERA_RAY : 0u));   // an entry of a ray queue is the ray (wavefront.h)
        pu(pool, F_FLAGS, s) = LF_ALIVE;   // (the traversal kernels and the fallback kernel read the queue entry alone)
    }
    const uint32_t full = e.quad_words;
    if (lds_depth == 0 || lds_depth > full) lds_depth = full;
    std::vector<uint32_t> overflow((size_t)(full + 64u) * blocks * TR_BLOCK, 0u);
    std::vector<uint32_t> fallback((size_t)n_slots * WF_RAY_WORDS, 0u);   // records of the deferred rays (on the device: the buffer of a ray queue that is idle during the stage)
    std::vector<DevStats> stats(WF_STAT_SLOTS);
    std::memset(stats.data(), 0, stats.size() * sizeof(DevStats));
    // (the traversal, then the rays it handed to the reference's binary traversal: round of wavefront_plan.h)
#define EMU_TRACE(S) do { launch(blocks, TR_BLOCK, [&] { k_wf_trace_dyn<S, 0>(e.d, pool, queue.data(), qctl.data(), stats.data(), lds_depth, overflow.data(), fallback.data(), 0u); }); \
                          launch(2, TR_BLOCK, [&] { k_wf_trace_fallback<S, 0>(e.d, pool, qctl.data(), fallback.data(), 0u); }); } while (0)
    if (stage == 0) EMU_TRACE(0); else if (stage == 1) EMU_TRACE(1); else EMU_TRACE(2);
#undef EMU_TRACE
    g_wf_deferred += qctl[WF_FB_WORD + stage];
    for (uint32_t s = 0; s < n; ++s) {
        const uint32_t fl = pu(pool, F_FLAGS, s);
        hit[s] = stage == 0 ? (fl & WF_HIT_A) != 0u : (stage == 1 ? (fl & WF_OCCLUDED) != 0u : (fl & WF_HIT_C) != 0u);
        t[s] = pf(pool, F_REC_T, s); inst[s] = pu(pool, F_REC_INST, s); prim[s] = pu(pool, F_REC_PRIM, s);
        b1[s] = pf(pool, F_REC_B1, s); b2[s] = pf(pool, F_REC_B2, s);
    }
    return 0;
}

// TRAYHIP_EMU_XF_TABLE=1: the frame's transform table (launch_buffers_plan.h: table_ensure; k_xf_table_build) under the emulated kernels. The table of all
// 2^24 shutter-time indices is 2 GB per moving instance: here it is a sparse mapping whose records exist for the indices the rendered (pixel, sample)
// pairs draw -- evaluated with k_xf_table_build's expressions --, which are the only ones the kernels read.
struct SparseXfTable {
    float* data = nullptr;
    size_t bytes = 0;
    uint32_t stride = 0;
    ~SparseXfTable() { if (data) munmap(data, bytes); }
    bool build(const TrayFlatScene* f, uint32_t frame, const uint32_t* moving_ids, uint32_t n_moving, const uint32_t* tiles_xy, uint32_t tile_count, uint32_t spp, uint64_t seed) {
        stride = n_moving + (f->camera.animated ? 1u : 0u);
        if (!stride) return true;
        bytes = ((size_t)1 << 24) * stride * TR_XF_REC * sizeof(float);
        void* p = mmap(nullptr, bytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
        if (p == MAP_FAILED) return false;
        data = static_cast<float*>(p);
        std::vector<uint8_t> have((size_t)1 << 21, 0u);   // one bit per index
        const uint32_t kf = tr_rules::frame_key(seed, frame);
        const TrayCamera& c = f->camera;
        for (uint32_t i = 0; i < tile_count; ++i)
            for (uint32_t pix = 0; pix < 64u; ++pix) {
                const uint32_t px = tiles_xy[2 * i] * 8u + (pix & 7u), py = tiles_xy[2 * i + 1] * 8u + (pix >> 3);   // (a queue entry is a tile's place in units of tiles)
                if (px >= f->film.width || py >= f->film.height) continue;
                const uint32_t kp = key_pixel(kf, py * f->film.width + px);
                for (uint32_t s = 0; s < spp; ++s) {
                    float x, y, t;
                    pixel_sample(kp, s, spp, px, py, x, y, t);
                    const uint32_t index = xf_time_index(t);
                    if (have[index >> 3] & (1u << (index & 7u))) continue;
                    have[index >> 3] |= (uint8_t)(1u << (index & 7u));
                    const float frame_time = (c.shutter_close - c.shutter_open) * xf_index_time(index) + c.shutter_open;   // (k_xf_table_build)
                    for (uint32_t m = 0; m < stride; ++m) {
                        uint32_t first, count;
                        if (m < n_moving) { const TrayInstance& in = f->instances[moving_ids[m]]; first = in.xf_first; count = in.xf_count; }
                        else { first = c.xf_first; count = c.xf_count; }
                        eval_xform_stack(f->xf_levels, f->keyframes, f->knots, first, count, frame_time, data + ((size_t)index * stride + m) * TR_XF_REC);
                    }
                }
            }
        return true;
    }
};

// The tile worker itself: k_path_tiles<0, FEAT> over `tile_count` tiles of the given Morton queue, launched the way
// launch_tiles does (feature set, light filter, stacks, row-binned film and cooperative small-mesh test are the scene's plan: scene_plan.h),
// as a SIMT emulation: 256 fibers per workgroup, wave intrinsics and barriers are rendezvous. rgbw is accumulated into.
// coop / film_rows: -1 = as the library decides, 0 = off. Returns 0, or -3 if a rendezvous could not complete.
// shard / n_shards / chunk_tiles: the launch tray_render_shard_device makes for one rank (chunks shard, shard + n_shards, ... of chunk_tiles
// tiles each); n_shards = 0 renders the whole queue given. [smp_begin, smp_end): the samples of the spp-sample frame to render, 0 / 0 = all of them.
static int render_tiles(const TrayFlatScene* f, const uint32_t* tiles_xy, uint32_t tile_count, uint32_t spp, uint32_t smp_begin, uint32_t smp_end, uint64_t seed,
                        float* rgbw, uint32_t blocks, int coop, int film_rows, unsigned long long* stats_out, uint32_t shard, uint32_t n_shards, uint32_t chunk_tiles) {
    EmuScene e;
    make_scene(f, e);
    const bool moving = e.plan.animated;
    if (f->n_instances > TR_FLAT_MAX && !moving) return -4;   // the library runs the wavefront schedule for those
    const uint32_t n_moving = e.plan.n_moving;
    const std::vector<uint32_t>& moving_ids = e.plan.moving_ids;
    std::vector<float> xf_cache;
    if (n_moving) {   // per-path transform cache, one column per thread of the grid
        xf_cache.assign((size_t)n_moving * TR_XF_WORDS * blocks * TR_BLOCK, 0.0f);
        e.d.xf_cache = xf_cache.data(); e.d.moving_ids = moving_ids.data(); e.d.n_moving = n_moving; e.d.xf_stride = n_moving; e.d.xf_cache_lanes = blocks * TR_BLOCK;
    }
    SparseXfTable table;   // TRAYHIP_EMU_XF_TABLE=1: the fill of the cache columns FROM THE TABLE (dev_geom.h: xf_cache_fill_wave, camera_ray) runs in the emulation
    if (moving && getenv("TRAYHIP_EMU_XF_TABLE") && atoi(getenv("TRAYHIP_EMU_XF_TABLE")) != 0) {
        if (!table.build(f, e.d.frame, moving_ids.data(), n_moving, tiles_xy, tile_count, spp, seed)) return -5;
        if (table.data) { e.d.moving_ids = moving_ids.data(); e.d.xf_tab = table.data; e.d.xf_tab_stride = table.stride; }
    }
    lds_layout(f, e, coop != 0, film_rows != 0);
    std::vector<uint2> tiles(tile_count);
    for (uint32_t i = 0; i < tile_count; ++i) tiles[i] = make_uint2(tiles_xy[2 * i], tiles_xy[2 * i + 1]);
    const tr_rules::TileWork w = n_shards ? tr_rules::shard_work(tile_count, shard, n_shards, chunk_tiles) : tr_rules::whole_queue(tile_count);   // tray_render_shard_device
    if (n_shards && w.work == 0u) { if (stats_out) stats_out[0] = stats_out[1] = stats_out[2] = stats_out[3] = 0; return 0; }
    uint32_t counter = 0;
    DevStats stats;
    std::memset(&stats, 0, sizeof stats);
    const uint32_t kf = tr_rules::frame_key(seed, e.d.frame);
    const int feat = e.plan.feat;
    tr_rules::whole_frame_range(spp, smp_begin, smp_end);
    const uint32_t levels = tr_rules::tile_levels(w.work, blocks, tr_rules::range_samples(spp, smp_begin, smp_end));
    int rc = 0;
    const auto run = [&](auto kernel) {
        rc = launch_simt(blocks, TR_BLOCK, [&] { kernel(e.d, tiles.data() + w.first, w.work, w.chunk, w.chunk_stride, spp, kf, levels, rgbw, &counter, &stats EMU_RANGE(smp_begin, smp_end)); },
                         e.plan.stack_bytes);
    };
    const bool whitted = e.d.integrator == TRAY_INTEGRATOR_WHITTED;
    if (moving) select_path_tiles<1>(feat, whitted, e.plan.light_filter, run); else select_path_tiles<0>(feat, whitted, e.plan.light_filter, run);
    if (stats_out) { stats_out[0] = stats.samples; stats_out[1] = stats.vertices; stats_out[2] = stats.rays; stats_out[3] = (unsigned long long)feat; }
    return rc;
}
int emu_render_tiles(const TrayFlatScene* f, const uint32_t* tiles_xy, uint32_t tile_count, uint32_t spp, uint64_t seed, float* rgbw,
                     uint32_t blocks, int coop, int film_rows, unsigned long long* stats_out, uint32_t shard, uint32_t n_shards, uint32_t chunk_tiles) {
    return render_tiles(f, tiles_xy, tile_count, spp, 0u, 0u, seed, rgbw, blocks, coop, film_rows, stats_out, shard, n_shards, chunk_tiles);
}

// The wavefront schedule as launch_wavefront of device_api.hip runs it -- the rules, the buffers' layout, a round's launches and the loop are the one
// copy in wavefront_plan.h -- as view 0 of 1 over an HBM-style path pool until every tile is done. What differs from the library is the emulation's own:
// the kernels run as SIMT emulations (EmuWfOps; `trace` is kept in the signature: 0 = k_wf_trace_dyn, the only traversal kernel), the buffers are
// vectors of the plan's sizes, and completion is looked at after every round, not every WF_POLL rounds. Moving scenes run the ANIM = 1 kernels with
// the per-slot transform cache.
// n_chunks = 256-slot chunks of the pool (<= tile_count); lds_depth as in emu_wf_trace. [smp_begin, smp_end): the samples of the spp-sample frame to
// render, 0 / 0 = all of them.
static int render_wavefront(const TrayFlatScene* f, const uint32_t* tiles_xy, uint32_t tile_count, uint32_t spp, uint32_t smp_begin, uint32_t smp_end, uint64_t seed,
                            float* rgbw, int trace, uint32_t n_chunks, uint32_t trace_blocks, uint32_t lds_depth, unsigned long long* stats_out) {
    EmuScene e;
    make_scene(f, e);
    const bool moving = e.plan.animated;
    const uint32_t n_moving = e.plan.n_moving;
    e.d.film_rows = e.plan.film_rows_ok ? 1u : 0u;
    tr_rules::whole_frame_range(spp, smp_begin, smp_end);
    const uint32_t n_smp = tr_rules::range_samples(spp, smp_begin, smp_end);
    const uint32_t slice_shift = tr_rules::wf_slice_shift(tile_count, n_chunks, n_smp, 0u);
    const uint32_t n_items = tile_count << slice_shift;
    n_chunks = std::max(1u, std::min(n_chunks, n_items));
    const uint32_t n_slots = n_chunks * TR_BLOCK;
    std::vector<float> pool_data((size_t)F_COUNT * n_slots, 0.0f);
    WfPool pool{pool_data.data(), n_slots, wf_seg_cap(n_chunks)};
    const std::vector<uint32_t>& moving_ids = e.plan.moving_ids;
    std::vector<float> xf_cache;
    if (n_moving) {   // per-path transform cache, one column per pool slot
        xf_cache.assign((size_t)n_moving * TR_XF_REC * n_slots, 0.0f);
        e.d.xf_cache = xf_cache.data(); e.d.moving_ids = moving_ids.data(); e.d.n_moving = n_moving; e.d.xf_stride = n_moving; e.d.xf_cache_lanes = n_slots; e.d.xf_aos = 1u;
    }
    SparseXfTable table;   // TRAYHIP_EMU_XF_TABLE=1: the stage kernels index the frame's table by the path's time index (device_api.hip: fill_launch_dev's wavefront branch)
    if (moving && getenv("TRAYHIP_EMU_XF_TABLE") && atoi(getenv("TRAYHIP_EMU_XF_TABLE")) != 0) {
        if (!table.build(f, e.d.frame, moving_ids.data(), n_moving, tiles_xy, tile_count, spp, seed)) return -5;
        if (table.data) {
            e.d.moving_ids = moving_ids.data(); e.d.n_moving = n_moving; e.d.xf_tab = table.data; e.d.xf_tab_stride = table.stride;
            e.d.xf_cache = table.data; e.d.xf_table = 1u; e.d.xf_aos = 1u; e.d.xf_stride = table.stride;
        }
    }
    std::vector<WfChunk> chunks(n_chunks, WfChunk{WF_TILE_NEED, 0u});
    std::vector<float> bins((size_t)n_chunks * ROWBIN_SIZE, 0.0f);
    uint32_t counters[2] = {0u, 0u};
    std::vector<DevStats> stats(WF_STAT_SLOTS);
    std::memset(stats.data(), 0, stats.size() * sizeof(DevStats));
    std::vector<uint2> tiles(tile_count);
    for (uint32_t i = 0; i < tile_count; ++i) tiles[i] = make_uint2(tiles_xy[2 * i], tiles_xy[2 * i + 1]);
    const uint32_t kf = tr_rules::frame_key(seed, e.d.frame);
    const uint32_t full = e.quad_words;
    if (lds_depth == 0 || lds_depth > full) lds_depth = full;
    trace_blocks = std::max(1u, std::min(trace_blocks, n_chunks));
    if (trace != 0) return -6;
    // the buffers, of the plan's sizes and cut as its view 0 of 1
    const tr_wfplan::Layout lay = tr_wfplan::layout(n_chunks, std::max(full, 8u), lds_depth, trace_blocks);
    const tr_wfplan::View view = tr_wfplan::view(lay, 0u, 1u, n_chunks);
    const bool sorted = !(e.plan.feat & FEAT_TEX);   // the material sort of the shading stage
    std::vector<uint32_t> queues(lay.queue_bytes / 4u, 0u), kind_queues(sorted ? lay.kind_bytes / 4u : 0u, 0u), bin_ctl(lay.bin_ctl_bytes / 4u, 0u), overflow(lay.ovf_bytes / 4u, 0u);
    const WfBinGrid bin_grid = f->n_top_nodes ? wf_bin_grid(f->top_nodes[0].bmin, f->top_nodes[0].bmax) : WfBinGrid{};
    EmuWfOps ops{e.d, pool, tr_wfplan::buffers(lay, view, queues.data(), sorted ? kind_queues.data() : nullptr, bin_ctl.data(), overflow.data()), chunks.data(), bins.data(),
                 tiles.data(), n_items, tile_count, spp, kf, rgbw, counters, stats.data(), slice_shift, smp_begin, smp_end, n_chunks, trace_blocks, lds_depth,
                 (size_t)e.plan.depth * TR_BLOCK * 4, (size_t)lay.bin_ctl_words, bin_grid};
    const tr_wfplan::RoundCfg cfg{sorted, tr_wfplan::fused_wanted(), tr_wfplan::bin_stages_wanted(), true, e.plan.mat_kinds_present};
    const uint64_t max_rounds = tr_wfplan::max_rounds(n_items, n_chunks, n_smp, slice_shift, e.d.max_depth);
    const auto poll = [&]() -> int { return ops.rc != 0 ? -1 : counters[1] >= n_items ? 1 : 0; };
    int rc = 0;
    uint64_t rounds = 0;
    if (counters[1] < n_items) {   // (a launch without work items runs no round)
        const tr_wfplan::Ended ended = moving ? tr_wfplan::run<1>(&ops, 1u, cfg, max_rounds, 1u, poll, &rounds) : tr_wfplan::run<0>(&ops, 1u, cfg, max_rounds, 1u, poll, &rounds);
        rc = ops.rc != 0 ? ops.rc : ended == tr_wfplan::kNotTerminated ? -5 : 0;   // -5: "wavefront schedule did not terminate"
    }
    if (stats_out) {
        DevStats st{};
        for (const DevStats& a : stats) { st.samples += a.samples; st.vertices += a.vertices; st.rays += a.rays; }
        stats_out[0] = st.samples; stats_out[1] = st.vertices; stats_out[2] = st.rays; stats_out[3] = rounds;
    }
    return rc;
}
int emu_render_wavefront(const TrayFlatScene* f, const uint32_t* tiles_xy, uint32_t tile_count, uint32_t spp, uint64_t seed, float* rgbw,
                         int trace, uint32_t n_chunks, uint32_t trace_blocks, uint32_t lds_depth, unsigned long long* stats_out) {
    return render_wavefront(f, tiles_xy, tile_count, spp, 0u, 0u, seed, rgbw, trace, n_chunks, trace_blocks, lds_depth, stats_out);
}

uint32_t emu_wf_bin_cells(void) { return 1u << WF_BIN_CELL_BITS; }
// The two binning kernels alone (tests/test_device_emulation.py): a queue of n_chunks x 256 slots whose segment `s` holds counts[s] ray records
// (8 words each, at queue[(s * seg_cap + k) * 8]); `sorted` receives every segment counting-sorted by wf_bin_key over the box (bmin, bmax), `keys`
// the key of every sorted entry. Returns the segments' capacity.
uint32_t emu_wf_bin(uint32_t n_chunks, const uint32_t* counts, const uint32_t* queue, uint32_t* sorted, uint32_t* keys, const float* bmin, const float* bmax, int stage) {
    WfPool pool{nullptr, n_chunks * TR_BLOCK, wf_seg_cap(n_chunks)};
    if (!queue) return pool.seg_cap;
    std::vector<uint32_t> qctl(WF_QCTL_WORDS, 0u), ctl((size_t)2u * WF_SEGS * WF_BINS, 0u);
    for (uint32_t s = 0; s < WF_SEGS; ++s) qctl[s * WF_SEG_STRIDE + (uint32_t)stage] = counts[s];
    const WfBinGrid g = wf_bin_grid(bmin, bmax);
    const uint32_t blocks = (pool.seg_cap + WF_BIN_EPB - 1u) / WF_BIN_EPB * WF_SEGS;
    int rc = 0;
    if (stage == 0) {
        rc = launch_simt(blocks, TR_BLOCK, [&] { k_wf_bin_hist<0>(pool, queue, qctl.data(), ctl.data(), g); });
        if (rc == 0) rc = launch_simt(blocks, TR_BLOCK, [&] { k_wf_bin_scatter<0>(pool, queue, sorted, qctl.data(), ctl.data(), g); });
    } else {
        rc = launch_simt(blocks, TR_BLOCK, [&] { k_wf_bin_hist<1>(pool, queue, qctl.data(), ctl.data(), g); });
        if (rc == 0) rc = launch_simt(blocks, TR_BLOCK, [&] { k_wf_bin_scatter<1>(pool, queue, sorted, qctl.data(), ctl.data(), g); });
    }
    if (rc != 0) return 0u;
    for (uint32_t s = 0; s < WF_SEGS; ++s)
        for (uint32_t k = 0; k < counts[s]; ++k) keys[(size_t)s * pool.seg_cap + k] = wf_bin_entry_key(g, sorted, (size_t)s * pool.seg_cap + k);
    return pool.seg_cap;
}

// The device films (kernels.hip) for samples of ONE tile (tx, ty), each sample written on its own into a zeroed image, and the
// image's pixels [floor(sx) - EMU_PATCH_R, floor(sx) + EMU_PATCH_R] x (the same in y) copied to out[i] (RGBW, zero off the image):
//   mode 0  film_splat into k_path_tiles' LDS window, flushed as k_path_tiles flushes it (TRAYHIP_DIRECT_FILM)
//   mode 1  film_splat_global (the wavefront film for filters without row bins; class-boundary samples of the row-binned films)
//   mode 2  film_splat_rows into the row bins, film_resolve_rows, the flush (k_path_tiles' row-binned film); 1 if the film has no row bins
//   mode 3  film_splat_rows_global<false> (the wavefront's row bins in global memory), film_resolve_rows, the flush; 1 as mode 2
//   mode 4  film_splat_window under the window of a group of group_w x group_h tiles aligned to multiples of the group (clipped to the
//           image's tiles, as the box of a ragged last group is), flushed as k_sampler_pass flushes it
// Returns 0; -1 if a write landed outside every patch or in the guard zones around the windows (an out-of-bounds LDS write on the device).
#define EMU_PATCH_R 6
int emu_film_splat(const TrayFilm* film, int mode, uint32_t tx, uint32_t ty, uint32_t group_w, uint32_t group_h, uint32_t n, const float* samples5, float* out) {
    DevScene d;
    std::memset(&d, 0, sizeof d);
    d.width = film->width; d.height = film->height;
    d.filter_w = film->filter_w; d.filter_h = film->filter_h; d.inv_w = film->inv_w; d.inv_h = film->inv_h;
    d.fpw = film->filter_pixel_w; d.fph = film->filter_pixel_h;
    d.filter_table = film->table; d.filter_x = film->table_x; d.filter_y = film->table_y;
    if ((mode == 2 || mode == 3) && !tr_plan::film_rows_ok(*film)) return 1;
    const int W = (int)film->width, H = (int)film->height, x0 = (int)tx * 8, y0 = (int)ty * 8;
    const size_t guard = 4096;
    std::vector<float> img((size_t)W * H * 4, 0.0f), win(guard + 4 * WIN_PLANE + guard, 0.0f), gwin(guard + 4 * SP_WIN_MAX * SP_WIN_MAX + guard, 0.0f);
    std::vector<float> bins(guard + ROWBIN_SIZE + guard, 0.0f);
    float* const s_win = win.data() + guard;
    float* const s_bins = bins.data() + guard;
    float* const s_gwin = gwin.data() + guard;
    // the group's window (k_sampler_pass: the box of its tiles, the filter's halo around it)
    const int ntx = W / 8, nty = H / 8;
    const int gx0 = (int)(tx / group_w * group_w), gy0 = (int)(ty / group_h * group_h);
    const int gx1 = std::min(gx0 + (int)group_w, ntx) - 1, gy1 = std::min(gy0 + (int)group_h, nty) - 1;
    const int gwx0 = gx0 * 8 - d.fpw, gwy0 = gy0 * 8 - d.fph;
    const int gww = (gx1 - gx0 + 1) * 8 + 2 * d.fpw + 1, gwh = (gy1 - gy0 + 1) * 8 + 2 * d.fph + 1;
    if (mode == 4 && (gww > SP_WIN_MAX || gwh > SP_WIN_MAX)) return -2;
    // flush of k_path_tiles' window (kernels.hip, after the tile's paths)
    auto flush_tile = [&]() {
        const int wx0 = x0 - d.fpw, wy0 = y0 - d.fph, ww = 8 + 2 * d.fpw + 1, wh = 8 + 2 * d.fph + 1;
        for (int i = 0; i < ww * wh; ++i) {
            const int wy = i / ww, wx = i - wy * ww, ix = wx0 + wx, iy = wy0 + wy;
            if (ix < 0 || iy < 0 || ix >= W || iy >= H) continue;
            const int o = wy * WIN_STRIDE + wx;
            float* dst = img.data() + ((size_t)iy * W + ix) * 4;
            for (int k = 0; k < 4; ++k) dst[k] += s_win[o + k * WIN_PLANE];
        }
        std::memset(s_win, 0, 4 * WIN_PLANE * sizeof(float));
    };
    for (uint32_t i = 0; i < n; ++i) {
        const float* s = samples5 + 5 * i;
        const float sx = s[0], sy = s[1];
        const f3 c = mk(s[2], s[3], s[4]);
        if (mode == 0) {
            film_splat(d, s_win, film->table, x0, y0, sx, sy, c);
            flush_tile();
        } else if (mode == 1) {
            film_splat_global(d, img.data(), film->table, x0, y0, sx, sy, c);
        } else if (mode == 2 || mode == 3) {
            const int py_l = (int)floorf(sy) - y0;
            if (mode == 2) film_splat_rows(d, s_bins, film->table_x, img.data(), film->table, x0, y0, py_l, sx, sy, c);
            else film_splat_rows_global<false>(d, s_bins, film->table_x, img.data(), film->table, x0, y0, py_l, sx, sy, c);
            for (uint32_t tid = 0; tid < TR_BLOCK; ++tid) film_resolve_rows(d, s_bins, film->table_y, s_win, y0, tid);
            std::memset(s_bins, 0, ROWBIN_SIZE * sizeof(float));
            flush_tile();
        } else if (mode == 4) {
            film_splat_window(d, s_gwin, gwx0, gwy0, gww, film->table, x0, y0, sx, sy, c);
            for (int k = 0; k < gww * gwh; ++k) {   // (k_sampler_pass's flush)
                const int wy = k / gww, wx = k - wy * gww, ix = gwx0 + wx, iy = gwy0 + wy;
                if (ix < 0 || iy < 0 || ix >= W || iy >= H) continue;
                float* dst = img.data() + ((size_t)iy * W + ix) * 4;
                for (int q = 0; q < 4; ++q) dst[q] += s_gwin[4 * k + q];
            }
            std::memset(s_gwin, 0, 4 * SP_WIN_MAX * SP_WIN_MAX * sizeof(float));
        } else {
            return -3;
        }
        const int cx = (int)floorf(sx), cy = (int)floorf(sy), P = 2 * EMU_PATCH_R + 1;
        float* o = out + (size_t)i * P * P * 4;
        std::memset(o, 0, (size_t)P * P * 4 * sizeof(float));
        for (int py = 0; py < P; ++py)
            for (int px = 0; px < P; ++px) {
                const int ix = cx - EMU_PATCH_R + px, iy = cy - EMU_PATCH_R + py;
                if (ix < 0 || iy < 0 || ix >= W || iy >= H) continue;
                float* src = img.data() + ((size_t)iy * W + ix) * 4;
                for (int k = 0; k < 4; ++k) { o[(py * P + px) * 4 + k] = src[k]; src[k] = 0.0f; }
            }
    }
    for (float v : img) if (v != 0.0f) return -1;
    for (const std::vector<float>* b : {&win, &gwin, &bins})
        for (size_t k = 0; k < b->size(); ++k) if ((*b)[k] != 0.0f) return -1;
    return 0;
}

}  // extern "C"

// The scene's plan (scene_plan.h) as the emulation applies it, for tests/test_scene_plan.py: its scalar fields in the order of tests/_emu.py's PLAN_FIELDS,
// then the constants the layout is made of. coop / film_rows as for emu_render_tiles.
extern "C" int emu_scene_plan(const TrayFlatScene* f, int coop, int film_rows, uint32_t* out) {
    EmuScene e;
    make_scene(f, e);
    lds_layout(f, e, coop != 0, film_rows != 0);
    const tr_plan::ScenePlan& p = e.plan;
    const uint32_t fields[] = {p.deforming, p.animated, (uint32_t)p.anim_debug(), (uint32_t)p.feat, p.light_filter, p.mat_kinds_present, p.film_rows_ok, p.wavefront,
                               p.mesh_depth, p.depth, p.coop_offset, p.win_offset, p.stack_bytes, p.n_moving, p.xf_movable,
                               TR_BLOCK, TR_COOP_MAX_TRIS, TR_COOP_WORDS, TR_FLAT_MAX, WIN_PLANE};
    std::memcpy(out, fields, sizeof fields);
    return 0;
}
// The device order of the trees and the wavefront traversal's instance records, as tray_scene_create uploads them (host/gates.hpp), for
// tests/test_device_tree_order.py. Two calls: with null outputs the counts come back (top nodes, mesh nodes, meshes, records).
extern "C" int emu_device_trees(const TrayFlatScene* f, uint32_t* counts, TrayBvhNode* top, TrayBvhNode* mesh, TrayMesh* meshes, void* wf_insts, int* narrow) {
    tray::PairedTrees p;
    if (!tray::pair_trees(f, p)) return 1;
    std::vector<tray::WfInst> recs;
    tray::QuadTrees q;
    tray::quad_trees(f, q);
    tray::wf_inst_records(f, q.mesh_first, recs);
    counts[0] = (uint32_t)p.top.size(); counts[1] = (uint32_t)p.mesh.size(); counts[2] = (uint32_t)p.meshes.size(); counts[3] = (uint32_t)recs.size();
    if (top) std::memcpy(top, p.top.data(), p.top.size() * sizeof(TrayBvhNode));
    if (mesh) std::memcpy(mesh, p.mesh.data(), p.mesh.size() * sizeof(TrayBvhNode));
    if (meshes) std::memcpy(meshes, p.meshes.data(), p.meshes.size() * sizeof(TrayMesh));
    if (wf_insts) std::memcpy(wf_insts, recs.data(), recs.size() * sizeof(tray::WfInst));
    if (narrow) *narrow = p.narrow ? 1 : 0;
    return 0;
}
// AnimatedTransform::transform(time) of a spline stack as the DEVICE evaluates it (dev_anim.h: eval_xform_stack): rows 0..2 of mat, rows 0..2 of inv
extern "C" int emu_stack_transform(const TrayFlatScene* f, uint32_t xf_first, uint32_t xf_count, uint32_t n, const float* times, float* out) {
    if (!f || (uint64_t)xf_first + xf_count > f->n_xf_levels) return -1;
    for (uint32_t k = 0; k < n; ++k) eval_xform_stack(f->xf_levels, f->keyframes, f->knots, xf_first, xf_count, times[k], out + (size_t)TR_XF_WORDS * k);
    return 0;
}
extern "C" unsigned emu_retraced(void) { const unsigned r = g_retraced; g_retraced = 0; return r; }
extern "C" unsigned emu_wf_deferred(void) { const unsigned r = g_wf_deferred; g_wf_deferred = 0; return r; }
// The wavefront traversal's quad records (host/gates.hpp: QuadTrees), for tests/test_device_tree_order.py. counts: top records, mesh records,
// meshes, top_pend, mesh_pend; null outputs = counts only. bfs_levels < 0: the library's default.
extern "C" int emu_quad_trees(const TrayFlatScene* f, int bfs_levels, uint32_t* counts, void* top, void* mesh, uint32_t* mesh_first, int* narrow) {
    tray::PairedTrees p;
    if (!tray::pair_trees(f, p)) return 1;
    tray::QuadTrees q;
    if (bfs_levels < 0) tray::quad_trees(f, q); else tray::quad_trees(f, q, false, (uint32_t)bfs_levels);
    counts[0] = (uint32_t)q.top.size(); counts[1] = (uint32_t)q.mesh.size(); counts[2] = (uint32_t)q.mesh_first.size(); counts[3] = q.top_pend; counts[4] = q.mesh_pend;
    if (top) std::memcpy(top, q.top.data(), q.top.size() * sizeof(tray::QuadNode));
    if (mesh) std::memcpy(mesh, q.mesh.data(), q.mesh.size() * sizeof(tray::QuadNode));
    if (mesh_first) std::memcpy(mesh_first, q.mesh_first.data(), q.mesh_first.size() * sizeof(uint32_t));
    if (narrow) *narrow = q.narrow ? 1 : 0;
    return 0;
}
