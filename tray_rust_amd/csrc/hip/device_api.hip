// Device-side C ABI of libtrayhip.so: device scenes (upload, frame update), the launches of the tile kernel / the wavefront schedule / the
// samplers, the transform table, the multi-device path (one stream per device + one RCCL sum-reduce), the debug entry points.
// The kernels themselves are kernels.hip + the dev_*.h / wavefront.h headers; their template instantiations are compiled in the objects of
// kernel_group.hip (kernel_list.h) -- this translation unit only DECLARES them, so a change here recompiles no kernel.
#include "kernels.hip"
#include <cmath>
#include <memory>
#define TR_INST_EXTERN   // explicit instantiation declarations of every kernel the launch sites below name
#include "kernel_list.h"
#include "kernel_select.h"   // (after the declarations: the selectors instantiate no kernel here)
#include "kernel_ranges.h"
#include "kernel_tiles.h"
#include "noise.h"
#include "nbound.h"
#include "denoise.h"
#include "guide.h"
#include "temporal.h"
#include "guided.h"
#include "first_hit.h"
#include "tdemod.h"
#include "t2pass.h"
#include "td2pass.h"
#undef TR_INST_EXTERN
#include "launch_rules.h"
#include "scene_plan.h"
#include "denoise_plan.h"
#include "noise_plan.h"
#include "wavefront_plan.h"   // (WF_PIPES_MAX, WF_POLL)
#include "launch_buffers_plan.h"


struct TrayDevBuf { const char* key; void* ptr; size_t bytes; };
// What tray_scene_update_frame requires of its argument: the SAME scene at another frame. The device buffers a frame update takes
// over without a copy (meshes, trees, triangles, MERL tables, textures, permutation pool, filter tables) are recognised by name and size
// only, so the sizes and parameters they depend on are recorded at creation and compared before anything is moved.
struct TraySceneIdentity {
    uint32_t n_instances, n_meshes, n_mesh_nodes, n_tris, n_materials, n_merl, n_textures, n_tex_frames, max_depth, min_depth, integrator, width, height;
    uint64_t n_merl_floats, n_tex_bytes;
    float filter[4];
    int32_t filter_px[2];
    uint32_t filter_hash;
    bool operator==(const TraySceneIdentity& o) const { return std::memcmp(this, &o, sizeof *this) == 0; }
};
static TraySceneIdentity scene_identity(const TrayFlatScene* f) {
    TraySceneIdentity id;
    std::memset(&id, 0, sizeof id);   // (padding bytes take part in the comparison)
    id.n_instances = f->n_instances; id.n_meshes = f->n_meshes; id.n_mesh_nodes = f->n_mesh_nodes; id.n_tris = f->n_tris; id.n_materials = f->n_materials;
    id.n_merl = f->n_merl; id.n_textures = f->n_textures; id.n_tex_frames = f->n_tex_frames; id.max_depth = f->max_depth; id.min_depth = f->min_depth;
    id.integrator = f->integrator; id.width = f->film.width; id.height = f->film.height;
    id.n_merl_floats = f->n_merl_floats; id.n_tex_bytes = f->n_tex_bytes;
    id.filter[0] = f->film.filter_w; id.filter[1] = f->film.filter_h; id.filter[2] = f->film.inv_w; id.filter[3] = f->film.inv_h;
    id.filter_px[0] = f->film.filter_pixel_w; id.filter_px[1] = f->film.filter_pixel_h;
    uint32_t h = 2166136261u;   // FNV-1a over the filter table's bits
    for (int k = 0; k < TRAY_FILTER_TABLE_SIZE * TRAY_FILTER_TABLE_SIZE; ++k) { uint32_t w; std::memcpy(&w, &f->film.table[k], 4); h = (h ^ w) * 16777619u; }
    id.filter_hash = h;
    return id;
}
// The three large buffers of a device scene's launches -- the wavefront pool with its queues, chunk records, row bins and overflow stacks; the per-path
// transform cache; the frame's transform table (dev_geom.h: xf_time_index). What they were sized for, and every decision to keep, drop or allocate one, is
// launch_buffers_plan.h's (st); LbOps below makes the HIP calls for it.
struct WfBuffers {   // the wavefront schedule's pool and the buffers that go with it (LbOps::grant_pool; 0.47 KB per slot)
    WfPool pool{nullptr, 0};
    WfChunk* d_chunks = nullptr;         // n_chunks of them, and as many row bins
    float* d_bins = nullptr;
    uint32_t n_chunks = 0;
    uint32_t *d_wf_counters = nullptr, *h_done = nullptr;   // [0] tile counter, [1] tiles done; pinned host mirror of tiles done
    uint32_t* d_queues = nullptr;        // ray queues A, B, C (n_slots each) + WF_QCTL_WORDS counters
    uint32_t* d_kind_queues = nullptr;   // WF_MAT_KINDS x n_slots slot indices
    uint32_t* d_bin_ctl = nullptr;       // ray binning before the traversal stages (wavefront.h: k_wf_bin_hist): per view and stage, histogram + cursors of every segment
    uint32_t* d_stack_overflow = nullptr;
    tr_wfplan::Layout lay{};             // where the views' parts of d_queues, d_kind_queues, d_bin_ctl and d_stack_overflow lie (wavefront_plan.h)
    uint32_t n_blocks_trace = 0;         // persistent grid of k_wf_trace_dyn
    uint32_t trace_lds_depth = 0, trace_lds_bytes = 0;   // LDS part of the dynamic-fetch kernel's stacks; deeper entries go to d_stack_overflow
    bool wf_sort = true;                 // material sort of the shading stage (k_wf_begin's LDS counting sort -> k_wf_query_kind); off for textured scenes
    std::vector<void*> allocs;           // the device buffers above
};
struct LaunchBuffers {
    tr_lbplan::State st;                 // which of the three exist, what they were sized for, what the last launch read
    WfBuffers wf;
    float* xf_cache = nullptr;           // the per-path transform cache (wavefront: one record of TR_XF_REC floats per pool slot and moving instance; tile kernel: one column per resident thread)
    float* d_xf_table = nullptr;         // the frame's transform table, built by the first launch that wants it
    hipEvent_t xf_table_ev = nullptr;    // recorded behind k_xf_table_build on xf_table_stream: a launch of the frame on ANOTHER stream waits for it
    hipStream_t xf_table_stream = nullptr;
};
// tray_render_noise_target_device's per-tile state in one allocation made on first use, laid out by noise_plan.h's tile_layout(n_tiles): the round's tile
// list (coordinates and queue indices; the error kernel reads it before the compaction rewrites it, in stream order, so one list serves every round), the
// next-round flags, the samples taken and the errors (by queue index), and the list's length; h_count is the pinned pair of words the host reads the
// round's counts through (the tile list's length; behind it, for the filtered rule, the block list's)
// bound: the neighbour bound's own buffers (tray_scene_set_noise_ratio; noise_plan.h's bound_layout), allocated by the first bounded call and anew when a
// call needs more; h_counts: the pinned words a bounded round's counts are read through (one per level list, and the block count)
struct NoiseBuffers {
    void* mem = nullptr;
    uint32_t* h_count = nullptr;
    void* bound = nullptr;
    uint64_t bound_bytes = 0;
    uint32_t* h_counts = nullptr;
};
struct TrayDeviceScene {
    int device = 0;
    DevScene dev{};
    std::vector<void*> allocs;
    std::vector<uint32_t> mesh_depths;   // deepest node of every BVH<Triangle> (scene_build: traversal stack size)
    std::vector<TrayDevBuf> bufs;        // the named uploads among `allocs`: what tray_scene_update_frame can carry over to the next frame
    TraySceneIdentity identity{};
    TrayDeviceScene* donor = nullptr;    // while a frame update builds the new state: the previous frame's scene, whose buffers may be taken
    bool broken = false;                 // a frame update failed half way: only tray_scene_destroy is valid
    uint2* d_tiles = nullptr;      // full Morton queue
    uint32_t n_tiles = 0;
    uint32_t* d_counter = nullptr;
    DevStats* d_stats = nullptr;
    uint32_t* d_retraced = nullptr;   // rays the flat instance loop re-traced through BVH<Instance> (dev_geom.h: trace)
    TrayInstance* d_instances = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timing_valid = false;
    bool empty_launch = false;           // the last render call had no tiles to render (reported as a launch of zero samples)
    uint32_t launches = 0;
    int n_blocks = 0;
    uint32_t n_materials = 0;
    LaunchBuffers lb;                    // wavefront pool, per-path transform cache, transform table
    uint32_t stack_bytes = 0;   // dynamic LDS of every kernel that traverses: stack depth x TR_BLOCK x 4
    bool wavefront = false;   // TRAYHIP_MODE=wave selects the stage-kernel schedule (wavefront.h)
    bool animated = false;    // something moves while the shutter is open: the <ANIM = true> kernels run
    uint32_t deferred_n_moving = 0;
    int feat = FEAT_ALL;              // lobe kinds of the scene's materials that need the large kernels (dev_bsdf.h)
    std::vector<TrayMesh> paired_meshes;   // the meshes with node_offset / node_count in device order (what the `meshes` buffer holds)
    std::vector<uint32_t> quad_first;      // per mesh: entry record of its tree in the `mesh_quads` buffer (host/gates.hpp: QuadTrees)
    size_t n_mesh_quads = 0;               // records of the BVH<Triangle>s at the head of the `quads` buffer
    uint32_t quad_mesh_pend = 0;           // most node entries a traversal of one BVH<Triangle>'s quad records can have pending
    uint32_t quad_stack_words = 0;         // stack words per lane the wavefront traversal needs for this frame's trees
    bool narrow_trees = true;         // every node's offset fits a descriptor (host/gates.hpp): the wavefront traversal keeps nodes as descriptors
    bool ordered_boxes = true;        // every BVH box has min <= max (host/gates.hpp: QuadTrees::ordered)
    DevScene launch_dev{};               // what the kernels of the current render call get: `dev` with the transform cache, or the table in its place (fill_launch_dev)
    bool camera_animated = false;
    uint32_t xf_movable = 0;             // instances (+ camera) whose transform has a level of several keyframes: what ANY frame of the sequence can move
    int xf_table_req = -1;               // tray_scene_set_transform_table: -1 = by the launch's sample count, 0 = never, 1 = always
    uint32_t wf_req_slots = 0, wf_req_views = 0, wf_req_slices = 0;   // tray_scene_set_wavefront: 0 = the library's own rule
    uint32_t last_views = 0, last_slices = 0;   // shape of the last wavefront launch (tray_last_schedule)
    bool last_was_wavefront = false;
    hipStream_t wf_streams[WF_PIPES_MAX] = {nullptr, nullptr, nullptr, nullptr};   // streams of views 1.. (view 0 runs on the caller's), created on first use
    hipEvent_t wf_fork = nullptr, wf_join[WF_PIPES_MAX] = {nullptr, nullptr, nullptr, nullptr};
    bool light_filter = false;        // a sphere light or specular lobes: the tile kernel with mis_ray_filter (dev_integrator.h) compiled in
    bool lean_tiles = true;           // whole-frame Path launches of a static scene run libtrayhip_tiles.so's kernel (kernel_tiles.h); TRAYHIP_LEAN_TILES=0: the base kernel
    WfBinGrid bin_grid{};                // the cells of the frame's BVH<Instance> box
    bool wf_fused = true;                // fused shading between the traversals (wavefront.h: k_wf_shade_kind); TRAYHIP_WF_FUSED=0|1 overrides
    uint32_t wf_bin_stages = 0u;         // bit 0: stage A rays are binned, bit 1: stage B rays (TRAYHIP_WF_BIN overrides)
    uint32_t mat_kinds_present = 0;   // bit per TRAY_MAT_* kind among the scene's materials
    // tray_scene_set_sampler: which Sampler the render calls stand for, and the per-pixel state of k_sampler_pass / k_sampler_decide
    bool deforming = false;           // the scene holds an AnimatedMesh: every render runs k_sampler_pass<3> (dev_geom.h: ANIM = 3), the debug kernels their <3> forms
    uint32_t sampler_kind = TRAY_SAMPLER_LOW_DISCREPANCY, smp_min = 1, smp_max = 1;
    void* d_smp = nullptr;            // [state u32 | running average f32 | luminances f32 x cap] per pixel of a batch of tiles
    size_t smp_bytes = 0;
    NoiseBuffers nt;                  // tray_render_noise_target_device (allocated on first use, kept across frame updates)
    uint32_t noise_ratio = 0;         // tray_scene_set_noise_ratio: 0 = no bound on the ratio of n_t between neighbouring tiles
    bool accumulate = false;          // a tray_render_noise_target_device call is running: its launches add to one set of stats, between its own events
};

static thread_local int g_device = 0;

#define HIP_CHECK(expr)                                                                                   \
    do {                                                                                                  \
        hipError_t _e = (expr);                                                                           \
        if (_e != hipSuccess) {                                                                           \
            set_error(std::string(#expr) + " failed: " + hipGetErrorString(_e));                          \
            return TRAY_E_DEVICE;                                                                         \
        }                                                                                                 \
    } while (0)

// Device copy of a host array under a name. During a frame update (s->donor set) a buffer of the same name and size is taken from
// the previous frame's scene instead of allocated: `unchanged` arrays (meshes, MERL tables, textures, the tile queue: the caller
// passes the same scene at another frame, tray_scene_update_frame) keep their content, the others are overwritten.
template <class T>
static int upload(TrayDeviceScene* s, const char* key, bool unchanged, const T* host, size_t n, const T** out) {
    *out = nullptr;
    size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    void* d = nullptr;
    bool reused = false;
    if (TrayDeviceScene* don = s->donor)
        for (size_t i = 0; i < don->bufs.size(); ++i)
            if (std::strcmp(don->bufs[i].key, key) == 0 && don->bufs[i].bytes == bytes) {
                d = don->bufs[i].ptr;
                don->allocs.erase(std::remove(don->allocs.begin(), don->allocs.end(), d), don->allocs.end());
                don->bufs.erase(don->bufs.begin() + (long)i);
                reused = true;
                break;
            }
    if (!d) HIP_CHECK(hipMalloc(&d, bytes));
    s->allocs.push_back(d);
    s->bufs.push_back(TrayDevBuf{key, d, bytes});
    if (!(reused && unchanged)) {
        if (n) HIP_CHECK(hipMemcpy(d, host, n * sizeof(T), hipMemcpyHostToDevice));
        else HIP_CHECK(hipMemset(d, 0, bytes));
    }
    *out = static_cast<const T*>(d);
    return TRAY_OK;
}


using tr_wfplan::QA; using tr_wfplan::QB; using tr_wfplan::QC; using tr_wfplan::QR; using tr_wfplan::Queue;
// What every view of a wavefront launch renders: the arguments of launch_wavefront
struct WfLaunch {
    const uint2* tiles;
    uint32_t tile_count, chunk, chunk_stride, spp, kf;   // tile_count: work items
    float* rgbw_dev;
    uint32_t slice_shift, smp_begin, smp_end;
};
// A view of the wavefront buffers (wavefront_plan.h: View) as the Ops of tr_wfplan::round: the plan's launch groups on the view's stream
struct WfOps {
    TrayDeviceScene* s;
    const WfLaunch* a;
    DevScene dev;       // the scene with xf_cache moved to the view's first slot
    WfPool pool;        // data moved to the view's first slot, n_slots = the pool's stride, seg_cap of the view's chunks
    WfChunk* chunks;
    float* bins;
    tr_wfplan::Buffers b;
    uint32_t n_chunks;
    hipStream_t stream;

    const WfBuffers& w() const { return s->lb.wf; }
    dim3 block() const { return dim3(TR_BLOCK); }
    dim3 grid() const { return dim3(n_chunks); }
    dim3 qgrid() const { return dim3((n_chunks + WF_SEGS - 1u) / WF_SEGS * WF_SEGS); }   // one-thread-per-entry kernels: block b reads segment b % WF_SEGS
    dim3 tgrid() const { return dim3(std::min<uint32_t>(w().n_blocks_trace, n_chunks)); }
    dim3 bgrid() const { return dim3((pool.seg_cap + WF_BIN_EPB - 1u) / WF_BIN_EPB * WF_SEGS); }
    uint32_t n_active() const { return n_chunks * TR_BLOCK; }
    uint32_t* qc(bool stage_c) const { return stage_c ? b.q[QC] : nullptr; }

    template <int ANIM> void advance() {
        uint32_t* const counters = w().d_wf_counters;
        if (a->smp_end) tr_ranges::wf_advance(ANIM, grid(), block(), stream, dev, pool, chunks, bins, a->tiles, a->tile_count, a->chunk, a->chunk_stride,   // (a sample range)
                                              a->spp, a->kf, a->rgbw_dev, counters, counters + 1, s->d_stats, b.q[QA], b.q[QR], b.qctl, a->slice_shift, a->smp_begin, a->smp_end);
        else hipLaunchKernelGGL(k_wf_advance<ANIM>, grid(), block(), 0, stream, dev, pool, chunks, bins, a->tiles, a->tile_count, a->chunk, a->chunk_stride,
                                a->spp, a->kf, a->rgbw_dev, counters, counters + 1, s->d_stats, b.q[QA], b.q[QR], b.qctl, a->slice_shift);
    }
    template <int ANIM> void regen() {
        hipLaunchKernelGGL(k_wf_regen<ANIM>, qgrid(), block(), 0, stream, dev, pool, chunks, a->tiles, a->chunk, a->chunk_stride, a->spp, a->kf, s->d_stats,
                           b.q[QR], b.q[QA], b.qctl, a->slice_shift);
    }
    template <int S> void bin(Queue from, Queue to) {
        uint32_t* const ctl = b.bin_ctl + (size_t)S * 2u * WF_SEGS * WF_BINS;
        hipLaunchKernelGGL(k_wf_bin_hist<S>, bgrid(), block(), 0, stream, pool, b.q[from], b.qctl, ctl, s->bin_grid);
        hipLaunchKernelGGL(k_wf_bin_scatter<S>, bgrid(), block(), 0, stream, pool, b.q[from], b.q[to], b.qctl, ctl, s->bin_grid);
    }
    template <int S, int ANIM> void trace(Queue from, Queue fallback, uint32_t fused) {
        hipLaunchKernelGGL((k_wf_trace_dyn<S, ANIM>), tgrid(), block(), w().trace_lds_bytes, stream, dev, pool, b.q[from], b.qctl, s->d_stats, w().trace_lds_depth, b.overflow, b.q[fallback], fused);
        hipLaunchKernelGGL((k_wf_trace_fallback<S, ANIM>), dim3(8), block(), s->stack_bytes, stream, dev, pool, b.qctl, b.q[fallback], fused);
    }
    int clear_qctl() { HIP_CHECK(hipMemsetAsync(b.qctl, 0, WF_QCTL_WORDS * sizeof(uint32_t), stream)); return TRAY_OK; }
    int clear_bin_ctl() { HIP_CHECK(hipMemsetAsync(b.bin_ctl, 0, (size_t)w().lay.bin_ctl_words * sizeof(uint32_t), stream)); return TRAY_OK; }
    void sort() { hipLaunchKernelGGL(k_wf_sort<0>, grid(), block(), 0, stream, dev, pool, n_active(), b.qctl, b.kq); }
    template <int ANIM, int K> void shade_kind() {
        hipLaunchKernelGGL((k_wf_shade_kind<ANIM, K>), qgrid(), block(), 0, stream, dev, pool, b.kq, b.qctl, s->d_stats, b.q[QA], b.q[QB]);
    }
    template <int ANIM> void begin() { hipLaunchKernelGGL(k_wf_begin<ANIM>, grid(), block(), 0, stream, dev, pool, n_active(), s->d_stats, b.q[QB], b.qctl, b.kq); }
    template <int ANIM, int K> void query_kind(bool stage_c) {
        hipLaunchKernelGGL((k_wf_query_kind<ANIM, K>), qgrid(), block(), 0, stream, dev, pool, b.kq, qc(stage_c), b.qctl, s->d_stats, b.q[QA]);
    }
    template <int ANIM> void query(bool stage_c) {
        hipLaunchKernelGGL((k_wf_query<ANIM, FEAT_ALL | FEAT_TEX>), grid(), block(), 0, stream, dev, pool, n_active(), qc(stage_c), b.qctl, s->d_stats, b.q[QA]);
    }
};

// the plain facts of the scene that launch_buffers_plan.h's rules are functions of
static tr_lbplan::Facts lb_facts(const TrayDeviceScene* s) {
    return tr_lbplan::Facts{s->n_tiles, (uint32_t)s->n_blocks, s->wavefront, s->animated, s->deferred_n_moving, s->stack_bytes, s->quad_stack_words,
                            s->xf_movable, s->camera_animated, s->wf_req_slots, s->xf_table_req};
}
// The Ops of launch_buffers_plan.h's procedures on a device scene: the HIP calls, the buffers' pointers, the error texts. stream: the launch's.
struct LbOps {
    TrayDeviceScene* s;
    hipStream_t stream = nullptr;

    bool free_bytes(uint64_t* out) {
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return false; }
        *out = free_b;
        return true;
    }
    bool grant_cache(uint32_t lanes, uint64_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) {
            (void)hipGetLastError();
            set_error("hipMalloc of the per-path transform cache failed: " + std::to_string(bytes >> 20) + " MiB for " + std::to_string(s->deferred_n_moving) +
                      " moving instances x " + std::to_string(lanes) + " paths (tray_scene_set_wavefront / TRAYHIP_WF_SLOTS / TRAYHIP_XF_CACHE_BYTES bound it)");
            return false;
        }
        s->lb.xf_cache = static_cast<float*>(p);
        return true;
    }
    bool grant_table(uint64_t bytes) {
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return false; }
        s->lb.d_xf_table = static_cast<float*>(p);
        return true;
    }
    // every buffer of the wavefront schedule for a pool of n_slots; on failure nothing stays allocated and TRAY_E_NOMEM is returned
    int grant_pool(uint32_t n_slots) {
        WfBuffers& w = s->lb.wf;
        auto grab = [&](uint64_t bytes, void** out) -> bool {
            void* p = nullptr;
            const hipError_t e = hipMalloc(&p, bytes);
            if (e != hipSuccess) {
                (void)hipGetLastError();
                set_error("hipMalloc of " + std::to_string(bytes >> 20) + " MiB failed: " + hipGetErrorString(e));
                drop(tr_lbplan::kPool);
                return false;
            }
            w.allocs.push_back(p);
            *out = p;
            return true;
        };
        void* p = nullptr;
        w.n_chunks = n_slots / TR_BLOCK;
        const uint32_t n_chunks = w.n_chunks;                    // (drop resets the fields on a failed grab)
        {   // the dynamic-fetch traversal's stacks and grid, then the shape of the queues and overflow columns they and the pool ask for (wavefront_plan.h)
            int per_cu = 0, cus = 256;
            hipDeviceProp_t prop;
            if (hipGetDeviceProperties(&prop, s->device) == hipSuccess && prop.multiProcessorCount > 0) cus = prop.multiProcessorCount;
            const uint32_t full_depth = tr_lbplan::trace_full_depth(s->quad_stack_words), lds_depth = tr_lbplan::trace_lds_depth(full_depth);
            w.trace_lds_depth = lds_depth;
            w.trace_lds_bytes = lds_depth * TR_BLOCK * (uint32_t)sizeof(uint32_t);
            hipError_t oe = s->animated ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_wf_trace_dyn<0, 1>, TR_BLOCK, w.trace_lds_bytes)
                                        : hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_wf_trace_dyn<0, 0>, TR_BLOCK, w.trace_lds_bytes);
            if (oe != hipSuccess || per_cu < 1) per_cu = 1;
            w.n_blocks_trace = (uint32_t)(cus * per_cu);
            w.lay = tr_wfplan::layout(n_chunks, full_depth, lds_depth, w.n_blocks_trace);
            if (getenv("TRAYHIP_STATS")) fprintf(stderr, "[trayhip] dynamic-fetch traversal: %u of %u stack entries in LDS, %d workgroups per CU\n", lds_depth, full_depth, per_cu);
        }
        const tr_wfplan::Layout lay = w.lay;
        if (!grab(tr_lbplan::pool_bytes(n_slots), &p)) return TRAY_E_NOMEM;
        w.pool.data = static_cast<float*>(p); w.pool.n_slots = n_slots; w.pool.seg_cap = wf_seg_cap(n_chunks);
        if (!grab(tr_lbplan::chunk_bytes(n_chunks), &p)) return TRAY_E_NOMEM;
        w.d_chunks = static_cast<WfChunk*>(p);
        if (!grab(tr_lbplan::bin_bytes(n_chunks), &p)) return TRAY_E_NOMEM;
        w.d_bins = static_cast<float*>(p);
        if (hipMemset(w.d_bins, 0, tr_lbplan::bin_bytes(n_chunks)) != hipSuccess) { set_error("hipMemset of the row bins failed"); drop(tr_lbplan::kPool); return TRAY_E_DEVICE; }
        if (!grab(2 * sizeof(uint32_t), &p)) return TRAY_E_NOMEM;
        w.d_wf_counters = static_cast<uint32_t*>(p);
        if (!grab(lay.queue_bytes, &p)) return TRAY_E_NOMEM;   // ray queues A, B, C, regeneration queue and the views' control words
        w.d_queues = static_cast<uint32_t*>(p);
        if (!grab(lay.bin_ctl_bytes, &p)) return TRAY_E_NOMEM;
        w.d_bin_ctl = static_cast<uint32_t*>(p);
        w.wf_sort = !(s->feat & FEAT_TEX);   // the kind-pure kernels read lobes from the material table; textured materials have theirs per hit
        if (w.wf_sort) {   // shading queues of the material sort
            if (!grab(lay.kind_bytes, &p)) return TRAY_E_NOMEM;
            w.d_kind_queues = static_cast<uint32_t*>(p);
        }
        if (!grab(lay.ovf_bytes, &p)) return TRAY_E_NOMEM;
        w.d_stack_overflow = static_cast<uint32_t*>(p);
        if (hipHostMalloc(reinterpret_cast<void**>(&w.h_done), sizeof(uint32_t), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); set_error("hipHostMalloc failed"); drop(tr_lbplan::kPool); return TRAY_E_NOMEM; }
        return TRAY_OK;
    }
    void drop(unsigned what) {
        LaunchBuffers& b = s->lb;
        if (what & tr_lbplan::kPool) {
            for (void* p : b.wf.allocs) (void)hipFree(p);
            if (b.wf.h_done) (void)hipHostFree(b.wf.h_done);
            b.wf = WfBuffers{};
        }
        if (what & tr_lbplan::kCache) {
            if (b.xf_cache) (void)hipFree(b.xf_cache);
            b.xf_cache = nullptr;
        }
        if (what & tr_lbplan::kTable) {
            if (b.d_xf_table) (void)hipFree(b.d_xf_table);
            if (b.xf_table_ev) (void)hipEventDestroy(b.xf_table_ev);
            b.d_xf_table = nullptr; b.xf_table_ev = nullptr; b.xf_table_stream = nullptr;
        }
    }
    int synchronise() { HIP_CHECK(hipDeviceSynchronize()); return TRAY_OK; }
    int table_build(uint32_t stride) {
        LaunchBuffers& b = s->lb;
        const uint32_t n_index = tr_lbplan::kTimeIndices;   // (the build reads moving_ids, instances, spline tables, camera of `dev`: none of them is a launch buffer)
        hipLaunchKernelGGL(k_xf_table_build, dim3(n_index / TR_BLOCK, stride), dim3(TR_BLOCK), 0, stream, s->dev, b.d_xf_table, stride, 0u, n_index);
        HIP_CHECK(hipGetLastError());
        // the build is ordered before this launch by the stream; the frame's later launches may come on other streams (tray_render_tiles_device /
        // tray_render_shard_device take the caller's): they wait for this event instead of reading a table that is still being written
        if (!b.xf_table_ev) HIP_CHECK(hipEventCreateWithFlags(&b.xf_table_ev, hipEventDisableTiming));
        HIP_CHECK(hipEventRecord(b.xf_table_ev, stream));
        b.xf_table_stream = stream;
        return TRAY_OK;
    }
    int table_wait() {
        if (stream != s->lb.xf_table_stream && s->lb.xf_table_ev) HIP_CHECK(hipStreamWaitEvent(stream, s->lb.xf_table_ev, 0));
        return TRAY_OK;
    }
    int refusal() {
        if (s->wavefront && !s->narrow_trees) { set_error("wavefront schedule: a BVH of more than 8 388 607 nodes or triangles (the traversal keeps a node as a 32-bit descriptor)"); return TRAY_E_UNSUPPORTED; }
        if (s->wavefront && !s->ordered_boxes) { set_error("wavefront schedule: a BVH box with min > max (or NaN) on some axis; TRAYHIP_MODE=mega renders such a scene with the tile kernel"); return TRAY_E_UNSUPPORTED; }
        return TRAY_OK;
    }
    void no_pool(uint32_t n_slots) {
        set_error("the wavefront schedule's buffers could not be allocated even for " + std::to_string(n_slots) + " pool slots (" +
                  std::to_string((n_slots * tr_lbplan::schedule_bytes_per_slot()) >> 20) + " MiB): " + tray_last_error());
    }
    void cache_short(uint32_t pool_slots, uint32_t lanes) {
        set_error("wavefront schedule: " + std::to_string(pool_slots) + " pool slots but a per-path transform cache of " + std::to_string(lanes) + " paths");
    }
};

extern "C" {

int tray_device_count(int* n) {
    if (!n) { set_error("tray_device_count: null argument"); return TRAY_E_INVALID; }
    hipError_t e = hipGetDeviceCount(n);
    if (e != hipSuccess) { *n = 0; set_error(std::string("hipGetDeviceCount failed: ") + hipGetErrorString(e)); return TRAY_E_DEVICE; }
    return TRAY_OK;
}

int tray_init(int device) {
    int n = 0;
    HIP_CHECK(hipGetDeviceCount(&n));
    if (device < 0 || device >= n) { set_error("tray_init: no such HIP device " + std::to_string(device)); return TRAY_E_INVALID; }
    HIP_CHECK(hipSetDevice(device));
    g_device = device;
    return TRAY_OK;
}

void tray_scene_destroy(TrayDeviceScene* s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    for (void* p : s->allocs) (void)hipFree(p);
    LbOps lb_ops{s};
    tr_lbplan::drop(lb_ops, s->lb.st, tr_lbplan::kAll);
    if (s->d_smp) (void)hipFree(s->d_smp);
    if (s->nt.mem) (void)hipFree(s->nt.mem);
    if (s->nt.h_count) (void)hipHostFree(s->nt.h_count);
    if (s->nt.bound) (void)hipFree(s->nt.bound);
    if (s->nt.h_counts) (void)hipHostFree(s->nt.h_counts);
    for (int k = 0; k < WF_PIPES_MAX; ++k) {
        if (s->wf_streams[k]) (void)hipStreamDestroy(s->wf_streams[k]);
        if (s->wf_join[k]) (void)hipEventDestroy(s->wf_join[k]);
    }
    if (s->wf_fork) (void)hipEventDestroy(s->wf_fork);
    if (s->ev0) (void)hipEventDestroy(s->ev0);
    if (s->ev1) (void)hipEventDestroy(s->ev1);
    delete s;
}

} // extern "C" (scene_build is internal)

// whether a whole-frame launch of this scene runs the lean tile kernel (kernel_tiles.h): static scenes under the Path integrator
static bool runs_lean_tiles(const TrayDeviceScene* s) {
    return s->lean_tiles && !s->animated && s->dev.integrator != TRAY_INTEGRATOR_WHITTED;
}

// the k_path_tiles instantiation launch_tiles runs for this scene: what the occupancy is asked of
static const void* tile_kernel(const TrayDeviceScene* s) {
    if (runs_lean_tiles(s)) return tr_tiles::path_tiles_kernel(s->feat, s->light_filter);
    const void* k = nullptr;
    const auto take = [&](auto kernel) { k = reinterpret_cast<const void*>(kernel); };
    const bool whitted = s->dev.integrator == TRAY_INTEGRATOR_WHITTED;
    if (s->animated) select_path_tiles<1>(s->feat, whitted, s->light_filter, take); else select_path_tiles<0>(s->feat, whitted, s->light_filter, take);
    return k;
}

// The trees of a scene in device order and what a frame update keeps of the donor's: host bookkeeping, nothing is uploaded here
struct SceneTrees {
    tray::PairedTrees paired;   // sibling pairs (host/gates.hpp); the BVH<Triangle>s are part of the scene, a frame update keeps the donor's
    tray::QuadTrees quads;      // the same trees as 128-byte records of two levels each, for the wavefront traversal (host/gates.hpp: QuadTrees)
    bool keep = false;
    size_t n_paired = 0;        // nodes of the BVH<Triangle>s in device order: one more per tree
    size_t top_quad_cap = 0;    // records a BVH<Instance> of this scene can need (one per interior node + the entry)
};
static int scene_trees(const TrayFlatScene* f, TrayDeviceScene* s, SceneTrees& t) {
    const TrayDeviceScene* donor = s->donor;
    for (uint32_t m = 0; m < f->n_meshes; ++m) t.n_paired += f->meshes[m].node_count ? f->meshes[m].node_count + 1u : 0u;
    t.top_quad_cap = 2u * (size_t)f->n_instances + 2u;
    if (donor && donor->quad_first.size() == f->n_meshes) {
        bool have_pairs = false, have_quads = false;
        for (const TrayDevBuf& b : donor->bufs) {
            have_pairs = have_pairs || (std::strcmp(b.key, "mesh_nodes") == 0 && b.bytes == std::max<size_t>(t.n_paired, 1) * sizeof(TrayBvhNode));
            have_quads = have_quads || (std::strcmp(b.key, "quads") == 0 && b.bytes == (donor->n_mesh_quads + t.top_quad_cap) * sizeof(tray::QuadNode));
        }
        t.keep = have_pairs && have_quads;
    }
    if (donor && !t.keep)
        if (const std::string bad = tray::validate_mesh_trees(f); !bad.empty()) { set_error("tray_scene_update_frame: inconsistent scene: " + bad); return TRAY_E_INVALID; }
    if (!tray::pair_trees(f, t.paired, t.keep)) { set_error("BVH arrays do not describe trees"); return TRAY_E_INVALID; }
    uint32_t bfs_levels = TRAY_QUAD_BFS_LEVELS;
    if (const char* e = getenv("TRAYHIP_QUAD_BFS")) bfs_levels = (uint32_t)std::max(0, atoi(e));
    tray::quad_trees(f, t.quads, t.keep, bfs_levels);
    s->narrow_trees = (t.keep ? donor->narrow_trees : t.paired.narrow) && t.quads.narrow;
    s->ordered_boxes = (t.keep ? donor->ordered_boxes : true) && t.quads.ordered;
    s->paired_meshes = t.keep ? donor->paired_meshes : t.paired.meshes;
    s->quad_first = t.keep ? donor->quad_first : t.quads.mesh_first;
    s->n_mesh_quads = t.keep ? donor->n_mesh_quads : t.quads.mesh.size();
    s->quad_mesh_pend = t.keep ? donor->quad_mesh_pend : t.quads.mesh_pend;
    // per lane: node entries are two words (descriptor, entry distance); the instances of a BVH<Instance> leaf (<= 31) and the
    // exit-mesh sentinel one each; rounded up so that consecutive frames of a sequence keep the pool's overflow columns
    s->quad_stack_words = (2u * (t.quads.top_pend + s->quad_mesh_pend) + 32u + 2u + 15u) / 16u * 16u;
    if (t.quads.top.size() > t.top_quad_cap || (s->n_mesh_quads + t.top_quad_cap) * sizeof(tray::QuadNode) >= ((size_t)1 << 32)) {
        set_error("the quad records of the scene's trees do not fit 32-bit offsets"); return TRAY_E_UNSUPPORTED;
    }
    // (a frame update that keeps the device's trees keeps their depths: tr_plan::mesh_depths)
    s->mesh_depths = t.keep && donor->mesh_depths.size() == f->n_meshes ? donor->mesh_depths : tr_plan::mesh_depths(f);
    return TRAY_OK;
}

// The decisions of scene_plan.h for this scene, with the environment's overrides, into the device scene
static int scene_plan(const TrayFlatScene* f, TrayDeviceScene* s, const std::vector<DevMaterial>& mats, tr_plan::ScenePlan& p) {
    tr_plan::plan_motion(f, p);
    if (p.n_moving > 64) { set_error("more than 64 instances move within one frame: the per-path transform cache does not cover that"); return TRAY_E_UNSUPPORTED; }
    tr_plan::plan_materials(mats, p);
    if (getenv("TRAYHIP_FEAT_ALL")) p.feat |= FEAT_ALL;
    tr_plan::plan_light_filter(f, p);
    if (getenv("TRAYHIP_NO_LIGHT_FILTER")) p.light_filter = false;
    p.film_rows_ok = tr_plan::film_rows_ok(f->film);
    s->dev.film_rows = (p.film_rows_ok && !getenv("TRAYHIP_DIRECT_FILM")) ? 1u : 0u;
    p.wavefront = tr_plan::wavefront(f, s->narrow_trees && s->ordered_boxes, p);
    if (const char* m = getenv("TRAYHIP_MODE")) p.wavefront = std::string(m) == "wave" && tr_plan::wavefront_can(f, p);   // (whatever the instance count and the trees)
    tr_plan::plan_stacks(f, s->mesh_depths, p);
    if (p.depth > 96) { set_error("BVH too deep for the LDS traversal stack (" + std::to_string(p.depth) + " levels)"); return TRAY_E_UNSUPPORTED; }
    if (getenv("TRAYHIP_STATS")) fprintf(stderr, "[trayhip] traversal stack: %u entries per lane (deepest BVH<Triangle> %u)\n", p.depth, p.mesh_depth);
    tr_plan::plan_lds(f, !getenv("TRAYHIP_NO_COOP"), s->dev.film_rows != 0u, p);
    s->deforming = p.deforming; s->animated = p.animated; s->deferred_n_moving = p.n_moving; s->xf_movable = p.xf_movable;
    s->feat = p.feat; s->light_filter = p.light_filter; s->mat_kinds_present = p.mat_kinds_present; s->wavefront = p.wavefront;
    s->stack_bytes = p.stack_bytes; s->dev.coop_offset = p.coop_offset; s->dev.win_offset = p.win_offset;
    // ray binning before the traversal stages (wavefront.h): the cells are those of the frame's BVH<Instance> root box
    s->bin_grid = f->n_top_nodes ? wf_bin_grid(f->top_nodes[0].bmin, f->top_nodes[0].bmax) : WfBinGrid{};
    s->wf_bin_stages = tr_wfplan::bin_stages_wanted();
    s->wf_fused = tr_wfplan::fused_wanted();
    if (const char* e = getenv("TRAYHIP_LEAN_TILES")) s->lean_tiles = atoi(e) != 0;   // (0: the base kernel, for A/B runs and bisecting)
    return TRAY_OK;
}

// The scene's device buffers (a frame update takes the donor's where upload() finds them) and the DevScene that points to them
static int scene_upload(const TrayFlatScene* f, TrayDeviceScene* s, const SceneTrees& t, const std::vector<DevMaterial>& mats, const tr_plan::ScenePlan& p) {
    DevScene& d = s->dev;
    int rc = TRAY_OK;
#define UP_(field, key, hostptr, count, unchanged)                                    \
    if (rc == TRAY_OK) {                                                              \
        std::remove_cv_t<std::remove_pointer_t<decltype(hostptr)>> const* _p = nullptr; \
        rc = upload(s, key, unchanged, hostptr, (size_t)(count), &_p);                \
        field = const_cast<std::remove_reference_t<decltype(field)>>(_p);             \
    }
#define UP(field, hostptr, count) UP_(d.field, #field, hostptr, count, false)    /* may differ from frame to frame */
#define UPS(field, hostptr, count) UP_(d.field, #field, hostptr, count, true)    /* part of the scene, the same at every frame */
    UP(instances, f->instances, f->n_instances)
    s->d_instances = const_cast<TrayInstance*>(d.instances);
    {   // the wavefront traversal's instance records (host/gates.hpp): per frame, as the instances are
        std::vector<tray::WfInst> recs;
        tray::wf_inst_records(f, s->quad_first, recs);
        UP(wf_insts, recs.data(), recs.size())
    }
    UP(top_nodes, t.paired.top.data(), t.paired.top.size())
    if (rc == TRAY_OK) {   // one buffer: the BVH<Triangle>s (kept across frames), then this frame's BVH<Instance>
        const tray::QuadNode* dq = nullptr;
        std::vector<tray::QuadNode> all;
        if (!t.keep) {
            all = t.quads.mesh;
            all.insert(all.end(), t.quads.top.begin(), t.quads.top.end());
            all.resize(s->n_mesh_quads + t.top_quad_cap, tray::quad_empty_record());
        }
        rc = upload(s, "quads", t.keep, t.keep ? static_cast<const tray::QuadNode*>(nullptr) : all.data(), s->n_mesh_quads + t.top_quad_cap, &dq);
        if (rc == TRAY_OK && t.keep && hipMemcpy(const_cast<tray::QuadNode*>(dq) + s->n_mesh_quads, t.quads.top.data(), t.quads.top.size() * sizeof(tray::QuadNode), hipMemcpyHostToDevice) != hipSuccess) {
            rc = TRAY_E_DEVICE; set_error("hipMemcpy of the BVH<Instance> records failed");
        }
        d.quads = reinterpret_cast<const float4*>(dq);
        d.top_quad_first = (uint32_t)s->n_mesh_quads;
    }
    UP(top_order, f->top_order, f->n_top_order)
    UPS(meshes, t.keep ? f->meshes : t.paired.meshes.data(), f->n_meshes)          // (kept: the donor's copies are not written)
    UPS(mesh_nodes, t.keep ? f->mesh_nodes : t.paired.mesh.data(), t.n_paired)
    UPS(tri_verts, f->tri_verts, f->n_tris)
    UPS(tri_attrs, f->tri_attrs, f->n_tris)
    UPS(mesh_keys, f->mesh_keys, f->n_mesh_keys)      // (AnimatedMesh: keyframe counts and times; read by the ANIM = 3 kernels only)
    UPS(key_times, f->key_times, f->n_key_times)
    if (f->n_textures) {
        UPS(textures, f->textures, f->n_textures)
        UPS(tex_frames, f->tex_frames, f->n_tex_frames)
        UPS(tex_data, f->tex_data, f->n_tex_bytes)
    }
    UP(materials, mats.data(), f->n_materials)
    UPS(merl_data, f->merl_data, f->n_merl_floats)
    UP(lights, f->lights, f->n_lights)
    UPS(filter_table, &f->film.table[0], TRAY_FILTER_TABLE_SIZE * TRAY_FILTER_TABLE_SIZE)
    UPS(filter_x, &f->film.table_x[0], TRAY_FILTER_TABLE_SIZE)
    UPS(filter_y, &f->film.table_y[0], TRAY_FILTER_TABLE_SIZE)
    UP(xf_levels, f->xf_levels, f->n_xf_levels)
    UP(keyframes, f->keyframes, f->n_keyframes)
    UP(knots, f->knots, f->n_knots)
    UP(color_keys, f->color_keys, f->n_color_keys)
    {   // the shuffles of the per-path LD arrays (path.rs:55-60: arrays of max_depth + 1 samples) come from a pool built once per scene
        std::vector<uint8_t> pool(TR_PERM_BYTES);
        perm_pool_build(f->max_depth + 1u, pool.data());
        UPS(perm_pool, pool.data(), pool.size())
    }
    {   // the flat instance loop's records and gates (host/gates.hpp; dev_geom.h: trace_flat, mesh_leaf_coop)
        std::vector<tray::FlatLeaf> leaves;
        std::vector<tray::FlatInst> insts;
        std::vector<uint8_t> tri_leaf;
        tray::flat_loop_gates(f, t.paired, TR_COOP_MAX_TRIS, leaves, insts, tri_leaf);
        UP(flat_leaves, leaves.data(), leaves.size())
        UP(flat_insts, insts.data(), insts.size())
        UPS(tri_leaf, tri_leaf.data(), tri_leaf.size())
        d.n_flat_leaves = (uint32_t)leaves.size();
    }
    UP_(d.camera_p, "camera", &f->camera, 1, false)
    s->camera_animated = f->camera.animated != 0;
    s->n_materials = f->n_materials;
    d.n_instances = f->n_instances; d.n_lights = f->n_lights; d.min_depth = f->min_depth; d.max_depth = f->max_depth;
    d.width = f->film.width; d.height = f->film.height; d.frame = f->frame; d.integrator = f->integrator;
    d.filter_w = f->film.filter_w; d.filter_h = f->film.filter_h; d.inv_w = f->film.inv_w; d.inv_h = f->film.inv_h;
    d.fpw = f->film.filter_pixel_w; d.fph = f->film.filter_pixel_h;
    // Morton tile queue (BlockQueue::new)
    if (rc == TRAY_OK) rc = tray_block_queue(d.width, d.height, 0, 0, nullptr, 0, &s->n_tiles);
    std::vector<uint32_t> xy(2 * (size_t)s->n_tiles);
    if (rc == TRAY_OK) rc = tray_block_queue(d.width, d.height, 0, 0, xy.data(), s->n_tiles, &s->n_tiles);
    UP_(s->d_tiles, "tiles", reinterpret_cast<const uint2*>(xy.data()), s->n_tiles, true)
    const uint32_t zero = 0;
    std::vector<DevStats> zs(WF_STAT_SLOTS);
    std::memset(zs.data(), 0, zs.size() * sizeof(DevStats));
    UP_(s->d_counter, "counter", &zero, 1, false)
    UP_(s->d_stats, "stats", zs.data(), zs.size(), false)
    UP_(s->d_retraced, "retraced", &zero, 1, false)
    d.retraced = s->d_retraced;
    if (rc == TRAY_OK && p.n_moving) {   // the moving instances of the per-path transform cache (dev_geom.h)
        UP_(d.moving_ids, "moving_ids", p.moving_ids.data(), p.moving_ids.size(), false)
        if (rc != TRAY_OK) rc = TRAY_E_NOMEM;
        d.n_moving = p.n_moving;
        d.xf_stride = p.n_moving;
        d.xf_aos = p.wavefront ? 1u : 0u;
    }
#undef UP
#undef UPS
#undef UP_
    if (rc != TRAY_OK) return rc;
    TrayDeviceScene* donor = s->donor;
    if (donor && donor->ev0 && donor->ev1) { s->ev0 = donor->ev0; s->ev1 = donor->ev1; donor->ev0 = nullptr; donor->ev1 = nullptr; }
    else if (hipEventCreate(&s->ev0) != hipSuccess || hipEventCreate(&s->ev1) != hipSuccess) { set_error("hipEventCreate failed"); return TRAY_E_DEVICE; }
    return TRAY_OK;
}

// Past the default dynamic-LDS window of 32 KB: raises the per-kernel limit (160 KB LDS per CU) of every kernel that is launched with the scene's
// stack_bytes (or its LDS part)
static void raise_lds_limit(uint32_t stack_bytes) {
    if (stack_bytes <= 32u * 1024u) return;
    const void* const traversing[] = {
        reinterpret_cast<const void*>(k_path_tiles<0, FEAT_NONE>), reinterpret_cast<const void*>(k_path_tiles<0, FEAT_MERL>),
        reinterpret_cast<const void*>(k_path_tiles<0, FEAT_SPEC>), reinterpret_cast<const void*>(k_path_tiles<0, FEAT_MERL | FEAT_SPEC>),
        reinterpret_cast<const void*>(k_path_tiles<0, FEAT_ALL>), reinterpret_cast<const void*>(k_path_tiles<1, FEAT_ALL>),
        reinterpret_cast<const void*>(k_path_tiles<0, FEAT_ALL | FEAT_TEX>), reinterpret_cast<const void*>(k_path_tiles<1, FEAT_ALL | FEAT_TEX>),
        reinterpret_cast<const void*>(k_path_tiles<1, FEAT_NONE>), reinterpret_cast<const void*>(k_path_tiles<1, FEAT_MERL>),
        reinterpret_cast<const void*>(k_path_tiles<1, FEAT_SPEC>), reinterpret_cast<const void*>(k_path_tiles<1, FEAT_MERL | FEAT_SPEC>),
        reinterpret_cast<const void*>(k_path_tiles<0, FEAT_NONE, TRAY_INTEGRATOR_PATH, true>), reinterpret_cast<const void*>(k_path_tiles<0, FEAT_MERL, TRAY_INTEGRATOR_PATH, true>), reinterpret_cast<const void*>(k_path_tiles<0, FEAT_SPEC, TRAY_INTEGRATOR_PATH, true>), reinterpret_cast<const void*>(k_path_tiles<0, FEAT_MERL | FEAT_SPEC, TRAY_INTEGRATOR_PATH, true>), reinterpret_cast<const void*>(k_path_tiles<0, FEAT_ALL, TRAY_INTEGRATOR_PATH, true>), reinterpret_cast<const void*>(k_path_tiles<0, FEAT_ALL | FEAT_TEX, TRAY_INTEGRATOR_PATH, true>),
        reinterpret_cast<const void*>(k_path_tiles<1, FEAT_NONE, TRAY_INTEGRATOR_PATH, true>), reinterpret_cast<const void*>(k_path_tiles<1, FEAT_MERL, TRAY_INTEGRATOR_PATH, true>), reinterpret_cast<const void*>(k_path_tiles<1, FEAT_SPEC, TRAY_INTEGRATOR_PATH, true>), reinterpret_cast<const void*>(k_path_tiles<1, FEAT_MERL | FEAT_SPEC, TRAY_INTEGRATOR_PATH, true>), reinterpret_cast<const void*>(k_path_tiles<1, FEAT_ALL, TRAY_INTEGRATOR_PATH, true>), reinterpret_cast<const void*>(k_path_tiles<1, FEAT_ALL | FEAT_TEX, TRAY_INTEGRATOR_PATH, true>),
        reinterpret_cast<const void*>(k_path_tiles<0, FEAT_ALL | FEAT_TEX, TRAY_INTEGRATOR_WHITTED>),
        reinterpret_cast<const void*>(k_path_tiles<1, FEAT_ALL | FEAT_TEX, TRAY_INTEGRATOR_WHITTED>),
        reinterpret_cast<const void*>(k_wf_trace_dyn<0, 0>), reinterpret_cast<const void*>(k_wf_trace_dyn<0, 1>),
        reinterpret_cast<const void*>(k_wf_trace_dyn<1, 0>), reinterpret_cast<const void*>(k_wf_trace_dyn<1, 1>),
        reinterpret_cast<const void*>(k_wf_trace_dyn<2, 0>), reinterpret_cast<const void*>(k_wf_trace_dyn<2, 1>),
        reinterpret_cast<const void*>(k_wf_trace_fallback<0, 0>), reinterpret_cast<const void*>(k_wf_trace_fallback<0, 1>),
        reinterpret_cast<const void*>(k_wf_trace_fallback<1, 0>), reinterpret_cast<const void*>(k_wf_trace_fallback<1, 1>),
        reinterpret_cast<const void*>(k_wf_trace_fallback<2, 0>), reinterpret_cast<const void*>(k_wf_trace_fallback<2, 1>),
        reinterpret_cast<const void*>(k_debug_intersect<0>), reinterpret_cast<const void*>(k_debug_intersect<2>),
        reinterpret_cast<const void*>(k_debug_sample_radiance<0>), reinterpret_cast<const void*>(k_debug_sample_radiance<2>),
        reinterpret_cast<const void*>(k_sampler_pass<0>), reinterpret_cast<const void*>(k_sampler_pass<2>), reinterpret_cast<const void*>(k_sampler_pass<3>),
        reinterpret_cast<const void*>(k_sampler_pass<0, FEAT_NONE>), reinterpret_cast<const void*>(k_sampler_pass<2, FEAT_NONE>), reinterpret_cast<const void*>(k_sampler_pass<3, FEAT_NONE>),
        reinterpret_cast<const void*>(k_debug_intersect<3>), reinterpret_cast<const void*>(k_debug_sample_radiance<3>)};
    for (const void* k : traversing) (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)stack_bytes);
    for (const int feat : {(int)FEAT_NONE, (int)FEAT_MERL, (int)FEAT_SPEC, FEAT_MERL | FEAT_SPEC, (int)FEAT_ALL, FEAT_ALL | FEAT_TEX})   // the lean tile kernels (kernel_tiles.h)
        for (const bool lf : {false, true}) (void)hipFuncSetAttribute(tr_tiles::path_tiles_kernel(feat, lf), hipFuncAttributeMaxDynamicSharedMemorySize, (int)stack_bytes);
    (void)hipGetLastError();
}

// workgroups of the persistent tile kernel: what fits the device, asked of the instantiation launch_tiles will run
static void scene_occupancy(TrayDeviceScene* s) {
    int per_cu = 0, cus = 0;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, s->device) == hipSuccess) cus = prop.multiProcessorCount;
    hipError_t occ = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, tile_kernel(s), TR_BLOCK, s->stack_bytes);
    if (occ != hipSuccess || per_cu < 1) per_cu = 1;
    if (cus < 1) cus = 256;
    s->n_blocks = cus * per_cu;
    if (getenv("TRAYHIP_STATS")) fprintf(stderr, "[trayhip] tile kernel: %d workgroups per CU (dynamic LDS %u B)\n", per_cu, s->stack_bytes);
}

static int scene_build(const TrayFlatScene* f, TrayDeviceScene* donor, TrayDeviceScene** out) {
    if (!f || !out) { set_error("tray_scene_create: null argument"); return TRAY_E_INVALID; }
    *out = nullptr;
    if (const tr_plan::Refusal no = tr_plan::refuse(f, donor == nullptr); no.rc != TRAY_OK) { set_error(no.msg); return no.rc; }
    std::unique_ptr<TrayDeviceScene, decltype(&tray_scene_destroy)> owner(new TrayDeviceScene(), tray_scene_destroy);   // (a step that fails destroys what was built)
    TrayDeviceScene* s = owner.get();
    s->identity = scene_identity(f);
    s->device = donor ? donor->device : g_device;
    s->donor = donor;
    if (hipSetDevice(s->device) != hipSuccess) { set_error("hipSetDevice failed (is a GPU present?)"); return TRAY_E_DEVICE; }
    SceneTrees trees;
    tr_plan::ScenePlan plan;
    std::vector<DevMaterial> mats(f->n_materials);
    for (uint32_t i = 0; i < f->n_materials; ++i) mats[i] = lower_material(f->materials[i], f->merl_tables);
    int rc = scene_trees(f, s, trees);
    if (rc == TRAY_OK) rc = scene_plan(f, s, mats, plan);
    if (rc == TRAY_OK) rc = scene_upload(f, s, trees, mats, plan);
    if (rc != TRAY_OK) return rc;
    raise_lds_limit(s->stack_bytes);
    scene_occupancy(s);
    {   // The launch buffers: the previous frame's in one move (freeing and allocating the 20 GB of a table costs 4 s -- profiles/r06_d_frame_overheads.txt --,
        // a pool seconds more), then the plan drops what this frame cannot use and allocates the tile kernel's cache
        s->wf_req_slots = donor ? donor->wf_req_slots : 0u; s->wf_req_views = donor ? donor->wf_req_views : 0u; s->wf_req_slices = donor ? donor->wf_req_slices : 0u;
        s->xf_table_req = donor ? donor->xf_table_req : -1;
        if (donor) s->lb = std::exchange(donor->lb, LaunchBuffers{});
        const uint32_t handed_slots = s->lb.st.pool_slots, handed_table_use = s->lb.st.last_used_table;   // (TRAYHIP_STATS)
        LbOps lb_ops{s};
        bool pool_kept = false;
        rc = tr_lbplan::frame(lb_ops, s->lb.st, lb_facts(s), &pool_kept);
        if (donor && getenv("TRAYHIP_STATS"))
            fprintf(stderr, "[trayhip] frame update: pool %s (donor ready %d, wavefront %d, stack %u / %u B, quad stack %u / %u, animated %d / %d, donor slots %u, cache lanes %u, donor used the table %d, table buffer %s)\n",
                    pool_kept ? "kept" : "not kept", handed_slots ? 1 : 0, s->wavefront ? 1 : 0, donor->stack_bytes, s->stack_bytes, donor->quad_stack_words, s->quad_stack_words,
                    donor->animated ? 1 : 0, s->animated ? 1 : 0, handed_slots, s->lb.st.cache_lanes, handed_table_use ? 1 : 0, s->lb.st.table ? "kept" : "none");
        if (rc != TRAY_OK) return rc;
    }
    s->donor = nullptr;
    *out = owner.release();
    return TRAY_OK;
}

extern "C" {

int tray_scene_create(const TrayFlatScene* f, TrayDeviceScene** out) { return scene_build(f, nullptr, out); }

// Scene::update_frame (scene.rs:152-176) for the device copy: the frame loop of main.rs:91-106 keeps the scene and rebuilds the
// instance transforms and BVH<Instance> per frame. `f` is the SAME scene flattened at another frame: meshes, MERL tables, textures,
// materials' tables and the tile queue are kept on the device (buffers whose size is unchanged are taken over without a copy),
// instances, BVH<Instance>, flat-loop records, camera, spline tables, colour keys and the moving set are uploaded anew, and the
// wavefront pool / queues and the per-path transform cache are carried over. Nothing else is assumed: every decision of
// tray_scene_create (schedule, kernel instantiation, stack depth, occupancy) is taken again for the new frame.
int tray_scene_update_frame(TrayDeviceScene* s, const TrayFlatScene* f) {
    if (!s || !f) { set_error("tray_scene_update_frame: null argument"); return TRAY_E_INVALID; }
    if (f->film.width != s->dev.width || f->film.height != s->dev.height) { set_error("tray_scene_update_frame: the film size changed: create a new device scene"); return TRAY_E_INVALID; }
    // nothing has moved yet: a scene that is not the one this copy was created from is refused and the handle stays usable
    if (!(scene_identity(f) == s->identity)) {
        set_error("tray_scene_update_frame: not the scene this device copy was created from (mesh / triangle / material / table counts, depths, integrator or filter differ)");
        return TRAY_E_INVALID;
    }
    HIP_CHECK(hipSetDevice(s->device));
    HIP_CHECK(hipDeviceSynchronize());   // (launches of the previous frame read the buffers that are about to be overwritten)
    TrayDeviceScene* n = nullptr;
    const int before = g_device;
    g_device = s->device;
    const size_t owned_before = s->allocs.size();
    const bool had_launch_buffers = s->lb.st.owns_any();
    const int rc = scene_build(f, s, &n);
    g_device = before;
    if (rc != TRAY_OK) {   // if a buffer has moved to the half-built (and now destroyed) new state the handle can only be destroyed; a refusal before that leaves it as it was
        s->donor = nullptr;
        if (s->allocs.size() != owned_before || (had_launch_buffers && !s->lb.st.owns_any())) s->broken = true;
        return rc;
    }
    n->sampler_kind = s->sampler_kind; n->smp_min = s->smp_min; n->smp_max = s->smp_max;   // (tray_scene_set_sampler belongs to the handle)
    n->noise_ratio = s->noise_ratio;   // (and so does tray_scene_set_noise_ratio)
    std::swap(n->d_smp, s->d_smp); std::swap(n->smp_bytes, s->smp_bytes);
    std::swap(n->nt, s->nt);
    std::swap(*s, *n);        // the handle keeps its identity; n now owns what the new frame did not take over
    tray_scene_destroy(n);
    return TRAY_OK;
}

// tiles: the launch's tile list in device memory (a sub-range of s->d_tiles, or tray_render_noise_target_device's list of active tiles); work item w renders
// tiles[(w / chunk) * chunk_stride * chunk + (w % chunk)].
// smp_begin / smp_end: the sample range [smp_begin, smp_end) of the spp-sample LowDiscrepancy frame to render (tray_render_samples_device); 0 / 0 = all of [0, spp)
static int launch_tiles(TrayDeviceScene* s, const uint2* tiles, uint32_t tile_count, uint32_t chunk, uint32_t chunk_stride,
                        uint32_t spp, uint64_t seed, float* rgbw_dev, void* stream_, uint32_t smp_begin = 0u, uint32_t smp_end = 0u);

// Wavefront schedule: rounds of six stage kernels over the path pool until every tile is done. The views, a round's launches and the loop are
// wavefront_plan.h's; what is this function's own: the streams and events of the views, their fork and join, the poll, the timing and the last_* fields.
static int launch_wavefront(TrayDeviceScene* s, const uint2* tiles, uint32_t tile_count, uint32_t chunk, uint32_t chunk_stride,
                            uint32_t spp, uint32_t kf, float* rgbw_dev, hipStream_t stream, uint32_t smp_begin, uint32_t smp_end) {
    const WfBuffers& w = s->lb.wf;
    const uint32_t n = tr_rules::range_samples(spp, smp_begin, smp_end);
    const uint32_t slice_shift = tr_rules::wf_slice_shift(tile_count, w.n_chunks, n, s->wf_req_slices);
    tile_count <<= slice_shift;   // from here on: work items
    const uint32_t n_chunks = std::min(w.n_chunks, tile_count);
    HIP_CHECK(hipMemsetAsync(w.d_wf_counters, 0, 2 * sizeof(uint32_t), stream));
        {   // chunks start in WF_TILE_NEED with done = 0
        std::vector<WfChunk> init(n_chunks, WfChunk{WF_TILE_NEED, 0u});
        HIP_CHECK(hipMemcpyAsync(w.d_chunks, init.data(), (size_t)n_chunks * sizeof(WfChunk), hipMemcpyHostToDevice, stream));
        HIP_CHECK(hipStreamSynchronize(stream));   // `init` is pageable host memory
    }
    if (!s->accumulate) HIP_CHECK(hipEventRecord(s->ev0, stream));
    const uint32_t n_views = tr_wfplan::view_count(n_chunks, s->wf_req_views);
    s->last_views = n_views; s->last_slices = 1u << slice_shift; s->last_was_wavefront = true;
    const WfLaunch args{tiles, tile_count, chunk, chunk_stride, spp, kf, rgbw_dev, slice_shift, smp_begin, smp_end};
    WfOps views[WF_PIPES_MAX];
    for (uint32_t k = 0; k < n_views; ++k) {
        const tr_wfplan::View pv = tr_wfplan::view(w.lay, k, n_views, n_chunks);
        WfOps& v = views[k];
        v.s = s; v.a = &args;
        v.n_chunks = pv.n_chunks;
        v.dev = s->launch_dev;
        if (v.dev.xf_cache && !v.dev.xf_table) v.dev.xf_cache += (size_t)pv.first_chunk * TR_BLOCK * v.dev.n_moving * TR_XF_REC;   // [slot][moving instance][TR_XF_REC] (the table is indexed by time, not by slot)
        v.pool = w.pool;
        v.pool.first = pv.first_chunk * TR_BLOCK;   // (the hit records are slot-major, the other fields field-major: the accessors add the view's first slot)
        v.pool.seg_cap = pv.seg_cap;
        v.chunks = w.d_chunks + pv.first_chunk;
        v.bins = w.d_bins + (size_t)pv.first_chunk * ROWBIN_SIZE;
        v.b = tr_wfplan::buffers(w.lay, pv, w.d_queues, w.wf_sort ? w.d_kind_queues : nullptr, w.d_bin_ctl, w.d_stack_overflow);
        v.stream = stream;
        if (k > 0) {   // (view 0 runs on the caller's stream)
            if (!s->wf_streams[k]) HIP_CHECK(hipStreamCreateWithFlags(&s->wf_streams[k], hipStreamNonBlocking));
            if (!s->wf_join[k]) HIP_CHECK(hipEventCreateWithFlags(&s->wf_join[k], hipEventDisableTiming));
            v.stream = s->wf_streams[k];
        }
    }
    if (n_views > 1u) {   // the other views start after what this call has put on the caller's stream so far
        if (!s->wf_fork) HIP_CHECK(hipEventCreateWithFlags(&s->wf_fork, hipEventDisableTiming));
        HIP_CHECK(hipEventRecord(s->wf_fork, stream));
        for (uint32_t k = 1; k < n_views; ++k) HIP_CHECK(hipStreamWaitEvent(views[k].stream, s->wf_fork, 0));
    }
    const tr_wfplan::RoundCfg cfg{w.wf_sort, s->wf_fused, s->wf_bin_stages, w.d_bin_ctl != nullptr, s->mat_kinds_present};
    const uint64_t max_rounds = tr_wfplan::max_rounds(tile_count, n_chunks, n, slice_shift, s->dev.max_depth);
    const auto poll = [&]() -> int {   // the "tiles done" word, once every view has drained
        HIP_CHECK(hipGetLastError());
        for (uint32_t k = 1; k < n_views; ++k) HIP_CHECK(hipStreamSynchronize(views[k].stream));
        HIP_CHECK(hipMemcpyAsync(w.h_done, w.d_wf_counters + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        return *w.h_done >= tile_count ? 1 : 0;
    };
    uint64_t rounds = 0;
    const tr_wfplan::Ended ended = s->animated ? tr_wfplan::run<1>(views, n_views, cfg, max_rounds, WF_POLL, poll, &rounds)
                                               : tr_wfplan::run<0>(views, n_views, cfg, max_rounds, WF_POLL, poll, &rounds);
    if (ended == tr_wfplan::kNotTerminated) { set_error("wavefront schedule did not terminate"); return TRAY_E_DEVICE; }
    if (ended == tr_wfplan::kFailed) return TRAY_E_DEVICE;   // (the failed call has set the error)
    for (uint32_t k = 1; k < n_views; ++k) {   // (the polls above have synchronised them; this keeps the caller's stream ordered after them in any case)
        HIP_CHECK(hipEventRecord(s->wf_join[k], views[k].stream));
        HIP_CHECK(hipStreamWaitEvent(stream, s->wf_join[k], 0));
    }
    HIP_CHECK(hipEventRecord(s->ev1, stream));
    s->timing_valid = true;
    s->launches = (uint32_t)(rounds * n_views * tr_wfplan::nominal_launches(s->wf_bin_stages));
    return TRAY_OK;
}

int tray_scene_set_sampler(TrayDeviceScene* s, uint32_t kind, uint32_t min_spp, uint32_t max_spp) {
    if (!s) { set_error("tray_scene_set_sampler: null argument"); return TRAY_E_INVALID; }
    if (kind > TRAY_SAMPLER_ADAPTIVE) { set_error("tray_scene_set_sampler: unknown sampler kind"); return TRAY_E_INVALID; }
    if (kind == TRAY_SAMPLER_ADAPTIVE) {
        if (min_spp > (1u << 16) || max_spp > (1u << 16)) { set_error("tray_scene_set_sampler: Adaptive takes at most 65 536 samples per pixel here"); return TRAY_E_UNSUPPORTED; }
        const uint32_t lo = tray_round_spp(min_spp), hi = tray_round_spp(max_spp);   // adaptive.rs:36-47
        if (hi < lo) { set_error("tray_scene_set_sampler: max_spp < min_spp (Adaptive::new would underflow, adaptive.rs:48)"); return TRAY_E_INVALID; }
        s->smp_min = lo; s->smp_max = hi;
    } else { s->smp_min = s->smp_max = 1u; }
    s->sampler_kind = kind;
    return TRAY_OK;
}

int tray_scene_set_noise_ratio(TrayDeviceScene* s, uint32_t max_ratio) {
    if (!s) { set_error("tray_scene_set_noise_ratio: null argument"); return TRAY_E_INVALID; }
    if (max_ratio != 0u && (max_ratio < 2u || max_ratio > (1u << 16) || (max_ratio & (max_ratio - 1u)) != 0u)) {
        set_error("tray_scene_set_noise_ratio: max_ratio must be 0 or a power of two in [2, 65536]"); return TRAY_E_INVALID;
    }
    s->noise_ratio = max_ratio;
    return TRAY_OK;
}

int tray_render_tiles_device(TrayDeviceScene* s, uint32_t tile_start, uint32_t tile_count, uint32_t spp, uint64_t seed,
                             float* rgbw_dev, void* stream_) {
    if (!s || !rgbw_dev) { set_error("tray_render_tiles_device: null argument"); return TRAY_E_INVALID; }
    tr_rules::clamp_tile_range(s->n_tiles, tile_start, tile_count);
    const tr_rules::TileWork w = tr_rules::whole_queue(tile_count);
    return launch_tiles(s, s->d_tiles + tile_start, w.work, w.chunk, w.chunk_stride, spp, seed, rgbw_dev, stream_);
}

int tray_render_shard_device(TrayDeviceScene* s, uint32_t shard, uint32_t n_shards, uint32_t chunk_tiles, uint32_t spp, uint64_t seed,
                             float* rgbw_dev, void* stream_) {
    if (!s || !rgbw_dev) { set_error("tray_render_shard_device: null argument"); return TRAY_E_INVALID; }
    if (n_shards == 0 || shard >= n_shards || chunk_tiles == 0) { set_error("tray_render_shard_device: bad shard / chunk arguments"); return TRAY_E_INVALID; }
    const tr_rules::TileWork w = tr_rules::shard_work(s->n_tiles, shard, n_shards, chunk_tiles);
    return launch_tiles(s, s->d_tiles + w.first, w.work, w.chunk, w.chunk_stride, spp, seed, rgbw_dev, stream_);
}

int tray_render_samples_device(TrayDeviceScene* s, uint32_t tile_start, uint32_t tile_count, uint32_t spp, uint32_t sample_begin, uint32_t sample_end,
                               uint64_t seed, float* rgbw_dev, void* stream_) {
    if (!s || !rgbw_dev) { set_error("tray_render_samples_device: null argument"); return TRAY_E_INVALID; }
    if (spp == 0 || (spp & (spp - 1)) != 0) { set_error("spp must be a power of two (LowDiscrepancy sampler, ld.rs:22-25); use tray_round_spp"); return TRAY_E_INVALID; }
    if (sample_begin >= sample_end || sample_end > spp) { set_error("tray_render_samples_device: the range must satisfy sample_begin < sample_end <= spp"); return TRAY_E_INVALID; }
    if (s->sampler_kind != TRAY_SAMPLER_LOW_DISCREPANCY) { set_error("tray_render_samples_device: sample ranges exist for the LowDiscrepancy sampler only"); return TRAY_E_UNSUPPORTED; }
    tr_rules::clamp_tile_range(s->n_tiles, tile_start, tile_count);
    const tr_rules::TileWork w = tr_rules::whole_queue(tile_count);
    return launch_tiles(s, s->d_tiles + tile_start, w.work, w.chunk, w.chunk_stride, spp, seed, rgbw_dev, stream_, sample_begin, sample_end);
}

// the ANIM argument of the debug, sampler and first-hit kernels
static int anim_debug(const TrayDeviceScene* s) { return tr_plan::anim_debug(s->deforming, s->animated); }

int tray_render_first_hit_device(TrayDeviceScene* s, uint32_t tile_start, uint32_t tile_count, uint32_t spp, uint32_t sample_begin, uint32_t sample_end,
                                 uint64_t seed, float* albedo_dev, float* normal_dev, float* depth_dev, void* stream_) {
    const std::string who("tray_render_first_hit_device");
    if (!s || !albedo_dev || !normal_dev || !depth_dev) { set_error(who + ": null argument"); return TRAY_E_INVALID; }
    if (spp == 0 || (spp & (spp - 1)) != 0) { set_error("spp must be a power of two (LowDiscrepancy sampler, ld.rs:22-25); use tray_round_spp"); return TRAY_E_INVALID; }
    if (sample_begin >= sample_end || sample_end > spp) { set_error(who + ": the range must satisfy sample_begin < sample_end <= spp"); return TRAY_E_INVALID; }
    const void* const films[3] = {albedo_dev, normal_dev, depth_dev};
    if (!tr_dnplan::distinct_aligned(films, 3u)) { set_error(who + ": the three films must be different buffers, 16-byte aligned"); return TRAY_E_INVALID; }
    if (s->sampler_kind != TRAY_SAMPLER_LOW_DISCREPANCY) { set_error(who + ": sample ranges exist for the LowDiscrepancy sampler only"); return TRAY_E_UNSUPPORTED; }
    if (s->broken) { set_error("this device scene is unusable: a tray_scene_update_frame on it failed"); return TRAY_E_INVALID; }
    tr_rules::clamp_tile_range(s->n_tiles, tile_start, tile_count);
    HIP_CHECK(hipSetDevice(s->device));
    if (tile_count == 0) return TRAY_OK;   // (an empty queue: nothing to add)
    // s->dev, not the launch copy: no per-path transform cache and no table, so the call needs none of a render's launch buffers
    tr_firsthit::tiles(anim_debug(s), static_cast<hipStream_t>(stream_), s->stack_bytes, s->dev, s->d_tiles + tile_start, tile_count, spp,
                       tr_rules::frame_key(seed, s->dev.frame), sample_begin, sample_end, albedo_dev, normal_dev, depth_dev);
    HIP_CHECK(hipGetLastError());
    return TRAY_OK;
}

// ---- the two noise-target calls. What each refuses, the layouts of the per-tile buffers and of the filtered rule's scratch, and the rounds with their
// one host read each are noise_plan.h's, shared with the host emulation; here the plan's schedule runs with launch_tiles and the add-on libraries'
// launch functions on the call's stream.

namespace nt = tr_ntplan;
static_assert(nt::kFinalFilterLaunches == tr_denoise::kLaunches && tr_dnplan::kPrepareLaunches == tr_denoise::kPrepareLaunches,
              "the plan counts the launches of a group as its library does");
static_assert(tr_guide::kBlockW == TRAY_DENOISE_BLOCK_W && tr_guide::kBlockH == TRAY_DENOISE_BLOCK_H, "the plan's blocks are the guide library's");

struct NoiseOps {   // the launch groups of the plan's schedule
    TrayDeviceScene* s;
    hipStream_t stream;
    uint64_t seed;
    uint32_t max_spp, width, height;
    static const uint2* xy(const void* tiles) { return static_cast<const uint2*>(tiles); }
    int render(const void* list, uint32_t n, uint32_t begin, uint32_t end, float* film, uint32_t* launches) {
        const int rc = launch_tiles(s, xy(list), n, n, 1u, max_spp, seed, film, stream, begin, end);
        if (rc == TRAY_OK) *launches += s->launches;
        return rc;
    }
    int block_list(const void* queue, const uint32_t* active, uint32_t n, uint32_t* flags, uint32_t* list, uint32_t* count) {
        HIP_CHECK(hipMemsetAsync(flags, 0, (size_t)nt::frame_blocks(width, height) * sizeof(uint32_t), stream));
        tr_guide::mark(stream, xy(queue), active, n, width, height, flags);
        tr_guide::compact(stream, flags, width, height, list, count);
        return TRAY_OK;
    }
    int halves(const float* even, const float* odd, void* records, uint32_t radius, uint32_t patch, float k, const uint32_t* blocks, uint32_t n_blocks,
               float* fa, float* fb) {
        tr_denoise::prepare(stream, even, odd, width, height, records);
        const uint32_t made = tr_guide::halves(stream, records, width, height, radius, patch, k, blocks, n_blocks, fa, fb);
        if (tr_denoise::kPrepareLaunches + made != nt::halves_launches(n_blocks)) {   // (the plan counts this group without asking)
            set_error("tray_render_noise_target_filtered_device: the halves made other launches than the plan counts"); return TRAY_E_DEVICE;
        }
        return TRAY_OK;
    }
    void error(const float* fe, const float* fo, const void* list, const uint32_t* list_q, uint32_t n, uint32_t taken, uint32_t max_spp_, float threshold,
               float* err, uint32_t* active, uint32_t* samples) {
        tr_noise::error(stream, fe, fo, width, height, xy(list), list_q, n, taken, max_spp_, threshold, err, active, samples);
    }
    void compact(const void* queue, const uint32_t* active, uint32_t n, void* list, uint32_t* list_q, uint32_t* count) {
        tr_noise::compact(stream, xy(queue), active, n, static_cast<uint2*>(list), list_q, count);
    }
    int read(const uint32_t* counts, uint32_t n_words, uint32_t* host) {   // through the scene's pinned words (a bounded call's: those of its own)
        uint32_t* const pinned = s->nt.h_counts ? s->nt.h_counts : s->nt.h_count;
        if (n_words > (s->nt.h_counts ? nt::kMaxLevels + 1u : 2u)) { set_error("a noise-target round reads more count words than the scene has pinned"); return TRAY_E_DEVICE; }
        HIP_CHECK(hipGetLastError());
        HIP_CHECK(hipMemcpyAsync(pinned, counts, n_words * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_CHECK(hipStreamSynchronize(stream));
        std::copy(pinned, pinned + n_words, host);
        return TRAY_OK;
    }
    // the neighbour bound's groups (libtrayhip_nbound.so)
    int grid(const void* queue, uint32_t n, uint32_t* map) {
        HIP_CHECK(tr_nbound::grid(stream, xy(queue), n, nt::grid_w(width), nt::grid_h(height), map));
        return TRAY_OK;
    }
    void pull(const void* queue, uint32_t n, const uint32_t* map, const uint32_t* samples, uint32_t* active, uint32_t max_ratio, uint32_t max_spp_) {
        tr_nbound::pull(stream, xy(queue), n, map, nt::grid_w(width), nt::grid_h(height), samples, active, max_ratio, max_spp_);
    }
    void compact_level(const void* queue, const uint32_t* active, const uint32_t* samples, uint32_t n_level, uint32_t n, void* list, uint32_t* list_q,
                       uint32_t* count) {
        tr_nbound::compact_level(stream, xy(queue), active, samples, n_level, n, static_cast<uint2*>(list), list_q, count);
    }
    int final_filter(const float* even, const float* odd, uint32_t radius, uint32_t patch, float k, float* out, void* records) {
        tr_denoise::denoise(stream, even, odd, width, height, radius, patch, k, out, records);
        HIP_CHECK(hipGetLastError());
        return TRAY_OK;
    }
};

static nt::Scene noise_scene(const TrayDeviceScene* s) {
    return s ? nt::Scene{true, s->sampler_kind, s->broken, s->dev.width, s->dev.height} : nt::Scene{false, 0u, false, 0u, 0u};
}

// The body of the two noise-target calls once their arguments are checked, what is HIP's of it: the per-tile buffers on first use, the call's events
// and statistics around the plan's rounds (f: the filtered rule's), and the per-tile results.
static int noise_target_call(TrayDeviceScene* s, uint32_t tile_start, uint32_t tile_count, uint32_t min_spp, uint32_t max_spp, float threshold, uint64_t seed,
                             float* even_dev, float* odd_dev, const nt::Filter* f, uint32_t* tile_samples, float* tile_error, void* stream_) {
    tr_rules::clamp_tile_range(s->n_tiles, tile_start, tile_count);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    HIP_CHECK(hipSetDevice(s->device));
    s->timing_valid = false;
    s->empty_launch = false;
    if (tile_count == 0) { std::fprintf(stderr, "Warning: This block queue is empty!\n"); s->empty_launch = true; return TRAY_OK; }   // block_queue.rs:42-44
    NoiseBuffers& b = s->nt;
    const nt::TileLayout tl = nt::tile_layout(s->n_tiles);
    if (!b.mem) HIP_CHECK(hipMalloc(&b.mem, (size_t)tl.total));
    if (!b.h_count) HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&b.h_count), 2u * sizeof(uint32_t), hipHostMallocDefault));
    // the neighbour bound (over two levels or more: one level has nothing to bound): its buffers on first use, anew if this call's levels need more
    nt::Bound bound{s->noise_ratio, nt::grid_w(s->dev.width), nt::grid_h(s->dev.height), nullptr};
    const bool bounded = s->noise_ratio != 0u && min_spp < max_spp;
    if (bounded) {
        const uint64_t need = nt::bound_layout(s->n_tiles, bound.grid_w, bound.grid_h, nt::levels_of(min_spp, max_spp)).total;
        if (b.bound && b.bound_bytes < need) { HIP_CHECK(hipStreamSynchronize(stream)); HIP_CHECK(hipFree(b.bound)); b.bound = nullptr; b.bound_bytes = 0; }
        if (!b.bound) { HIP_CHECK(hipMalloc(&b.bound, (size_t)need)); b.bound_bytes = need; }
        if (!b.h_counts) HIP_CHECK(hipHostMalloc(reinterpret_cast<void**>(&b.h_counts), (nt::kMaxLevels + 1u) * sizeof(uint32_t), hipHostMallocDefault));
        bound.mem = b.bound;
    }
    HIP_CHECK(hipMemsetAsync(s->d_stats, 0, WF_STAT_SLOTS * sizeof(DevStats), stream));   // (the launches below add to them: s->accumulate)
    HIP_CHECK(hipMemsetAsync(s->d_retraced, 0, sizeof(uint32_t), stream));
    HIP_CHECK(hipEventRecord(s->ev0, stream));
    uint32_t launches = 0u;
    NoiseOps ops{s, stream, seed, max_spp, s->dev.width, s->dev.height};
    s->accumulate = true;
    const nt::Refusal no = nt::run(ops, nt::Target{s->d_tiles + tile_start, tile_count, min_spp, max_spp, threshold, even_dev, odd_dev, b.mem, s->n_tiles}, f, &launches,
                                   bounded ? &bound : nullptr);
    s->accumulate = false;
    if (no.rc != TRAY_OK) {   // (a failed call has set the error itself; the renders before it have set timing_valid)
        if (!no.msg.empty()) set_error(no.msg);
        s->timing_valid = false;
        return no.rc;
    }
    HIP_CHECK(hipEventRecord(s->ev1, stream));
    HIP_CHECK(hipMemcpyAsync(tile_samples, nt::at(b.mem, tl.samples), (size_t)tile_count * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipMemcpyAsync(tile_error, nt::at(b.mem, tl.err), (size_t)tile_count * sizeof(float), hipMemcpyDeviceToHost, stream));
    HIP_CHECK(hipStreamSynchronize(stream));
    s->launches = launches;
    s->timing_valid = true;
    return TRAY_OK;
}

int tray_render_noise_target_device(TrayDeviceScene* s, uint32_t tile_start, uint32_t tile_count, uint32_t min_spp, uint32_t max_spp, float threshold,
                                    uint64_t seed, float* even_dev, float* odd_dev, uint32_t* tile_samples, float* tile_error, void* stream_) {
    const nt::Refusal no = nt::target_rules("tray_render_noise_target_device", noise_scene(s), min_spp, max_spp, threshold, even_dev, odd_dev, tile_samples, tile_error);
    if (no.rc != TRAY_OK) { set_error(no.msg); return no.rc; }
    if (const nt::Refusal nb = nt::bound_rules("tray_render_noise_target_device", s->noise_ratio, min_spp, max_spp); nb.rc != TRAY_OK) { set_error(nb.msg); return nb.rc; }
    return noise_target_call(s, tile_start, tile_count, min_spp, max_spp, threshold, seed, even_dev, odd_dev, nullptr, tile_samples, tile_error, stream_);
}

uint64_t tray_noise_target_filtered_scratch_bytes(uint32_t width, uint32_t height) { return nt::filtered_scratch_bytes(width, height); }

int tray_render_noise_target_filtered_device(TrayDeviceScene* s, uint32_t tile_start, uint32_t tile_count, uint32_t min_spp, uint32_t max_spp, float threshold,
                                             uint64_t seed, float* even_dev, float* odd_dev, uint32_t radius, uint32_t patch, float k, float* out_dev,
                                             void* scratch_dev, uint32_t* tile_samples, float* tile_error, void* stream_) {
    const nt::Refusal no = nt::filtered_rules("tray_render_noise_target_filtered_device", noise_scene(s), min_spp, max_spp, threshold, even_dev, odd_dev, radius,
                                              patch, k, out_dev, scratch_dev, tile_samples, tile_error);
    if (no.rc != TRAY_OK) { set_error(no.msg); return no.rc; }
    if (const nt::Refusal nb = nt::bound_rules("tray_render_noise_target_filtered_device", s->noise_ratio, min_spp, max_spp); nb.rc != TRAY_OK) { set_error(nb.msg); return nb.rc; }
    const nt::Filter f{radius, patch, k, scratch_dev, out_dev};
    return noise_target_call(s, tile_start, tile_count, min_spp, max_spp, threshold, seed, even_dev, odd_dev, &f, tile_samples, tile_error, stream_);
}

// ---- the thirteen tray_denoise_*_device calls. What each refuses, its scratch layout and its launches in order are denoise_plan.h's, shared with the
// host emulation; here the plan's schedules run with the add-on libraries' launch functions on the call's stream.

namespace dn = tr_dnplan;
static_assert(dn::kPrepareLaunches == tr_denoise::kPrepareLaunches && dn::kDenoiseLaunches == tr_denoise::kLaunches &&
              dn::kDemodLaunches == tr_firsthit::kDemodLaunches, "the plan counts the launches of a group as its library does");

struct DenoiseOps {   // the launch groups of the plan's schedules
    hipStream_t stream;
    uint32_t width, height;
    void prepare(const float* even, const float* odd, void* records) { tr_denoise::prepare(stream, even, odd, width, height, records); }
    void denoise(const float* even, const float* odd, uint32_t radius, uint32_t patch, float k, float* out, void* scratch) {
        tr_denoise::denoise(stream, even, odd, width, height, radius, patch, k, out, scratch);
    }
    void halves(const void* records, uint32_t radius, uint32_t patch, float k, const uint32_t* blocks, uint32_t n_blocks, float* fa, float* fb) {
        tr_guide::halves(stream, records, width, height, radius, patch, k, blocks, n_blocks, fa, fb);
    }
    void filter(const void* guide, const void* values, uint32_t radius, uint32_t patch, float k, float* out) {
        tr_guided::filter(stream, guide, values, width, height, radius, patch, k, out);
    }
    void temporal_pass(const void* centre, const void* frame, uint32_t radius, uint32_t patch, float k, void* sums, bool first, bool last, float* out) {
        tr_temporal::pass(stream, centre, frame, width, height, radius, patch, k, sums, first, last, out);
    }
    void tdemod_prepare(const float* even, const float* odd, const float* albedo, void* records) {
        tr_tdemod::prepare(stream, even, odd, albedo, width, height, records);
    }
    void tdemod_pass(const void* centre, const void* frame, const float* albedo, uint32_t radius, uint32_t patch, float k, void* sums, bool first, bool last,
                     float* out) {
        tr_tdemod::pass(stream, centre, frame, albedo, width, height, radius, patch, k, sums, first, last, out);
    }
    void t2_halves_pass(const void* centre, const void* frame, uint32_t radius, uint32_t patch, float k, void* sums, bool first, bool last, float* fa, float* fb) {
        tr_t2pass::halves_pass(stream, centre, frame, width, height, radius, patch, k, sums, first, last, fa, fb);
    }
    void t2_guided_pass(const void* centre_guide, const void* guide, const void* values, uint32_t radius, uint32_t patch, float k, void* sums, bool first,
                        bool last, float* out) {
        tr_t2pass::guided_pass(stream, centre_guide, guide, values, width, height, radius, patch, k, sums, first, last, out);
    }
    void td2_prepare(const float* even, const float* odd, const float* albedo, void* records) {
        tr_td2pass::prepare(stream, even, odd, albedo, width, height, records);
    }
    void td2_guided_pass(const void* centre_guide, const void* guide, const void* values, const float* albedo, uint32_t radius, uint32_t patch, float k,
                         void* sums, bool first, bool last, float* out) {
        tr_td2pass::guided_pass(stream, centre_guide, guide, values, albedo, width, height, radius, patch, k, sums, first, last, out);
    }
    void demodulate(const float* even, const float* odd, const float* albedo, float* even_out, float* odd_out) {
        tr_firsthit::demodulate(stream, even, odd, albedo, width, height, even_out, odd_out);
    }
    void remodulate(const float* albedo, float* out) { tr_firsthit::remodulate(stream, albedo, width, height, out); }
};

// a call once the plan has judged its arguments: the refusal, or the schedule on the library's current device
extern "C++" template <class Schedule>
static int denoise_call(const dn::Refusal& no, uint32_t width, uint32_t height, void* stream_, Schedule&& schedule) {
    if (no.rc != TRAY_OK) { set_error(no.msg); return no.rc; }
    HIP_CHECK(hipSetDevice(g_device));
    DenoiseOps ops{static_cast<hipStream_t>(stream_), width, height};
    schedule(ops);
    HIP_CHECK(hipGetLastError());
    return TRAY_OK;
}

int tray_denoise_halves_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev, uint32_t radius, uint32_t patch, float k,
                               const uint32_t* blocks_dev, uint32_t n_blocks, float* fa_dev, float* fb_dev, void* scratch_dev, void* stream_) {
    const dn::Frame f{even_dev, odd_dev, nullptr, nullptr, nullptr};
    const dn::Params p{radius, 0u, patch, k};
    const dn::Refusal no = dn::halves_rules(width, height, f, p, blocks_dev, n_blocks, tr_guide::blocks_x(width) * tr_guide::blocks_y(height), fa_dev, fb_dev,
                                            scratch_dev);
    if (no.rc != TRAY_OK) { set_error(no.msg); return no.rc; }
    HIP_CHECK(hipSetDevice(g_device));
    if (blocks_dev && n_blocks == 0u) return TRAY_OK;   // (nothing to compute: no launch at all)
    DenoiseOps ops{static_cast<hipStream_t>(stream_), width, height};
    dn::halves(ops, f, p, blocks_dev, n_blocks, fa_dev, fb_dev, scratch_dev);
    HIP_CHECK(hipGetLastError());
    return TRAY_OK;
}

uint64_t tray_denoise_scratch_bytes(uint32_t width, uint32_t height) { return dn::plain_layout(width, height).total; }

int tray_denoise_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev, uint32_t radius, uint32_t patch, float k,
                        float* out_dev, void* scratch_dev, void* stream_) {
    const dn::Frame f{even_dev, odd_dev, nullptr, nullptr, nullptr};
    const dn::Params p{radius, 0u, patch, k};
    return denoise_call(dn::denoise_rules(width, height, even_dev, odd_dev, p, out_dev, scratch_dev), width, height, stream_,
                        [&](DenoiseOps& ops) { dn::denoise(ops, f, p, out_dev, scratch_dev); });
}

uint64_t tray_denoise_temporal_scratch_bytes(uint32_t width, uint32_t height) { return dn::temporal_layout(width, height).total; }

int tray_denoise_temporal_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev, uint32_t n_neighbours,
                                 const float* const* nb_even_dev, const float* const* nb_odd_dev, uint32_t radius, uint32_t radius_t, uint32_t patch, float k,
                                 float* out_dev, void* scratch_dev, void* stream_) {
    const dn::Frame f{even_dev, odd_dev, nullptr, nullptr, nullptr};
    const dn::Neighbours nb{n_neighbours, nb_even_dev, nb_odd_dev, nullptr, nullptr, nullptr};
    const dn::Params p{radius, radius_t, patch, k};
    return denoise_call(dn::temporal_rules(width, height, f, nb, p, out_dev, scratch_dev), width, height, stream_,
                        [&](DenoiseOps& ops) { dn::temporal(ops, f, nb, p, out_dev, scratch_dev); });
}

uint64_t tray_denoise_guided_scratch_bytes(uint32_t width, uint32_t height) { return dn::guided_layout(width, height).total; }

int tray_denoise_guided_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev, const float* guide_a_dev, const float* guide_b_dev,
                               uint32_t radius, uint32_t patch, float k, float* out_dev, void* scratch_dev, void* stream_) {
    const dn::Frame f{even_dev, odd_dev, nullptr, guide_a_dev, guide_b_dev};
    const dn::Params p{radius, 0u, patch, k};
    return denoise_call(dn::guided_rules(width, height, f, p, out_dev, scratch_dev), width, height, stream_,
                        [&](DenoiseOps& ops) { dn::guided(ops, f, p, out_dev, scratch_dev); });
}

uint64_t tray_denoise_two_pass_scratch_bytes(uint32_t width, uint32_t height) { return dn::two_pass_layout(width, height).total; }

int tray_denoise_two_pass_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev, uint32_t radius, uint32_t patch, float k,
                                 uint32_t radius2, uint32_t patch2, float k2, float* out_dev, void* scratch_dev, void* stream_) {
    const dn::Frame f{even_dev, odd_dev, nullptr, nullptr, nullptr};
    const dn::Params p{radius, 0u, patch, k}, second{radius2, 0u, patch2, k2};
    return denoise_call(dn::two_pass_rules(width, height, f, p, second, out_dev, scratch_dev), width, height, stream_,
                        [&](DenoiseOps& ops) { dn::two_pass(ops, f, p, second, out_dev, scratch_dev); });
}

uint64_t tray_denoise_demodulated_scratch_bytes(uint32_t width, uint32_t height, uint32_t radius2) {
    return dn::demodulated_layout(width, height, radius2 != 0u).total;
}

int tray_denoise_demodulated_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev, const float* albedo_dev, uint32_t radius,
                                    uint32_t patch, float k, uint32_t radius2, uint32_t patch2, float k2, float* out_dev, void* scratch_dev, void* stream_) {
    const dn::Frame f{even_dev, odd_dev, albedo_dev, nullptr, nullptr};
    const dn::Params p{radius, 0u, patch, k}, second_pass{radius2, 0u, patch2, k2};
    const dn::Params* const second = radius2 != 0u ? &second_pass : nullptr;   // (radius2 == 0: one pass)
    return denoise_call(dn::demodulated_rules(width, height, f, p, second, out_dev, scratch_dev), width, height, stream_,
                        [&](DenoiseOps& ops) { dn::demodulated(ops, f, p, second, out_dev, scratch_dev); });
}

uint64_t tray_denoise_temporal_demodulated_scratch_bytes(uint32_t width, uint32_t height) { return dn::temporal_layout(width, height).total; }

int tray_denoise_temporal_demodulated_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev, const float* albedo_dev,
                                             uint32_t n_neighbours, const float* const* nb_even_dev, const float* const* nb_odd_dev,
                                             const float* const* nb_albedo_dev, uint32_t radius, uint32_t radius_t, uint32_t patch, float k, float* out_dev,
                                             void* scratch_dev, void* stream_) {
    const dn::Frame f{even_dev, odd_dev, albedo_dev, nullptr, nullptr};
    const dn::Neighbours nb{n_neighbours, nb_even_dev, nb_odd_dev, nb_albedo_dev, nullptr, nullptr};
    const dn::Params p{radius, radius_t, patch, k};
    return denoise_call(dn::temporal_demodulated_rules(width, height, f, nb, p, out_dev, scratch_dev), width, height, stream_,
                        [&](DenoiseOps& ops) { dn::temporal_demodulated(ops, f, nb, p, out_dev, scratch_dev); });
}

uint64_t tray_denoise_temporal_halves_scratch_bytes(uint32_t width, uint32_t height) { return dn::temporal_layout(width, height).total; }

int tray_denoise_temporal_halves_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev, uint32_t n_neighbours,
                                        const float* const* nb_even_dev, const float* const* nb_odd_dev, uint32_t radius, uint32_t radius_t, uint32_t patch,
                                        float k, float* fa_dev, float* fb_dev, void* scratch_dev, void* stream_) {
    const dn::Frame f{even_dev, odd_dev, nullptr, nullptr, nullptr};
    const dn::Neighbours nb{n_neighbours, nb_even_dev, nb_odd_dev, nullptr, nullptr, nullptr};
    const dn::Params p{radius, radius_t, patch, k};
    return denoise_call(dn::temporal_halves_rules(width, height, f, nb, p, fa_dev, fb_dev, scratch_dev), width, height, stream_,
                        [&](DenoiseOps& ops) { dn::temporal_halves(ops, f, nb, p, fa_dev, fb_dev, scratch_dev); });
}

uint64_t tray_denoise_temporal_guided_scratch_bytes(uint32_t width, uint32_t height) { return dn::temporal_guided_layout(width, height).total; }

int tray_denoise_temporal_guided_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev, const float* guide_a_dev,
                                        const float* guide_b_dev, uint32_t n_neighbours, const float* const* nb_even_dev, const float* const* nb_odd_dev,
                                        const float* const* nb_guide_a_dev, const float* const* nb_guide_b_dev, uint32_t radius, uint32_t radius_t,
                                        uint32_t patch, float k, float* out_dev, void* scratch_dev, void* stream_) {
    const dn::Frame f{even_dev, odd_dev, nullptr, guide_a_dev, guide_b_dev};
    const dn::Neighbours nb{n_neighbours, nb_even_dev, nb_odd_dev, nullptr, nb_guide_a_dev, nb_guide_b_dev};
    const dn::Params p{radius, radius_t, patch, k};
    return denoise_call(dn::temporal_guided_rules(width, height, f, nb, p, out_dev, scratch_dev), width, height, stream_,
                        [&](DenoiseOps& ops) { dn::temporal_guided(ops, f, nb, p, out_dev, scratch_dev); });
}

uint64_t tray_denoise_temporal_two_pass_scratch_bytes(uint32_t width, uint32_t height) { return dn::temporal_two_pass_layout(width, height).total; }

int tray_denoise_temporal_two_pass_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev, uint32_t n_neighbours,
                                          const float* const* nb_even_dev, const float* const* nb_odd_dev, uint32_t radius, uint32_t radius_t, uint32_t patch,
                                          float k, uint32_t radius2, uint32_t radius_t2, uint32_t patch2, float k2, float* out_dev, void* scratch_dev,
                                          void* stream_) {
    const dn::Frame f{even_dev, odd_dev, nullptr, nullptr, nullptr};
    const dn::Neighbours nb{n_neighbours, nb_even_dev, nb_odd_dev, nullptr, nullptr, nullptr};
    const dn::Params p{radius, radius_t, patch, k}, second{radius2, radius_t2, patch2, k2};
    return denoise_call(dn::temporal_two_pass_rules(width, height, f, nb, p, second, out_dev, scratch_dev), width, height, stream_,
                        [&](DenoiseOps& ops) { dn::temporal_two_pass(ops, f, nb, p, second, out_dev, scratch_dev); });
}

// the two-pass temporal filter on albedo-demodulated films: the three calls above with every frame's films resolved through its albedo

uint64_t tray_denoise_temporal_demodulated_halves_scratch_bytes(uint32_t width, uint32_t height) { return dn::temporal_layout(width, height).total; }

int tray_denoise_temporal_demodulated_halves_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev, const float* albedo_dev,
                                                    uint32_t n_neighbours, const float* const* nb_even_dev, const float* const* nb_odd_dev,
                                                    const float* const* nb_albedo_dev, uint32_t radius, uint32_t radius_t, uint32_t patch, float k,
                                                    float* fa_dev, float* fb_dev, void* scratch_dev, void* stream_) {
    const dn::Frame f{even_dev, odd_dev, albedo_dev, nullptr, nullptr};
    const dn::Neighbours nb{n_neighbours, nb_even_dev, nb_odd_dev, nb_albedo_dev, nullptr, nullptr};
    const dn::Params p{radius, radius_t, patch, k};
    return denoise_call(dn::temporal_demodulated_halves_rules(width, height, f, nb, p, fa_dev, fb_dev, scratch_dev), width, height, stream_,
                        [&](DenoiseOps& ops) { dn::temporal_demodulated_halves(ops, f, nb, p, fa_dev, fb_dev, scratch_dev); });
}

uint64_t tray_denoise_temporal_demodulated_guided_scratch_bytes(uint32_t width, uint32_t height) { return dn::temporal_guided_layout(width, height).total; }

int tray_denoise_temporal_demodulated_guided_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev, const float* albedo_dev,
                                                    const float* guide_a_dev, const float* guide_b_dev, uint32_t n_neighbours,
                                                    const float* const* nb_even_dev, const float* const* nb_odd_dev, const float* const* nb_albedo_dev,
                                                    const float* const* nb_guide_a_dev, const float* const* nb_guide_b_dev, uint32_t radius,
                                                    uint32_t radius_t, uint32_t patch, float k, float* out_dev, void* scratch_dev, void* stream_) {
    const dn::Frame f{even_dev, odd_dev, albedo_dev, guide_a_dev, guide_b_dev};
    const dn::Neighbours nb{n_neighbours, nb_even_dev, nb_odd_dev, nb_albedo_dev, nb_guide_a_dev, nb_guide_b_dev};
    const dn::Params p{radius, radius_t, patch, k};
    return denoise_call(dn::temporal_demodulated_guided_rules(width, height, f, nb, p, out_dev, scratch_dev), width, height, stream_,
                        [&](DenoiseOps& ops) { dn::temporal_demodulated_guided(ops, f, nb, p, out_dev, scratch_dev); });
}

uint64_t tray_denoise_temporal_demodulated_two_pass_scratch_bytes(uint32_t width, uint32_t height) {
    return dn::temporal_two_pass_layout(width, height).total;
}

int tray_denoise_temporal_demodulated_two_pass_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev, const float* albedo_dev,
                                                      uint32_t n_neighbours, const float* const* nb_even_dev, const float* const* nb_odd_dev,
                                                      const float* const* nb_albedo_dev, uint32_t radius, uint32_t radius_t, uint32_t patch, float k,
                                                      uint32_t radius2, uint32_t radius_t2, uint32_t patch2, float k2, float* out_dev, void* scratch_dev,
                                                      void* stream_) {
    const dn::Frame f{even_dev, odd_dev, albedo_dev, nullptr, nullptr};
    const dn::Neighbours nb{n_neighbours, nb_even_dev, nb_odd_dev, nb_albedo_dev, nullptr, nullptr};
    const dn::Params p{radius, radius_t, patch, k}, second{radius2, radius_t2, patch2, k2};
    return denoise_call(dn::temporal_demodulated_two_pass_rules(width, height, f, nb, p, second, out_dev, scratch_dev), width, height, stream_,
                        [&](DenoiseOps& ops) { dn::temporal_demodulated_two_pass(ops, f, nb, p, second, out_dev, scratch_dev); });
}


int tray_multi_shard_samples(uint32_t spp, uint32_t d, uint32_t n_dev, uint32_t* begin, uint32_t* end) {
    if (!begin || !end) { set_error("tray_multi_shard_samples: null argument"); return TRAY_E_INVALID; }
    if (spp == 0 || (spp & (spp - 1)) != 0) { set_error("spp must be a power of two (LowDiscrepancy sampler, ld.rs:22-25); use tray_round_spp"); return TRAY_E_INVALID; }
    if (n_dev == 0 || d >= n_dev) { set_error("tray_multi_shard_samples: device index out of range"); return TRAY_E_INVALID; }
    *begin = (uint32_t)((uint64_t)d * spp / n_dev);
    *end = (uint32_t)((uint64_t)(d + 1u) * spp / n_dev);
    return TRAY_OK;
}

// thread_work with sampler::Uniform / sampler::Adaptive (include/trayhip.h: tray_scene_set_sampler): rounds of k_sampler_pass (+
// k_sampler_decide) over batches of tiles, all on `stream`, no host synchronisation -- a pixel that is finished sits out the later rounds.
static int launch_sampler(TrayDeviceScene* s, const uint2* tiles, uint32_t tile_count, uint32_t chunk, uint32_t chunk_stride,
                          uint32_t spp, uint32_t kf, float* rgbw_dev, hipStream_t stream, uint32_t smp_begin, uint32_t smp_end) {
    SamplerPass sp{};
    sp.kind = s->sampler_kind; sp.min_spp = s->smp_min; sp.max_spp = s->smp_max;
    const uint32_t rounds = tr_rules::sampler_plan(sp, spp);
    // tiles per batch: the per-pixel state within 256 MB and the largest round within 2^28 threads
    const size_t px_bytes = 8u + 4u * (size_t)sp.lum_cap;
    const uint32_t widest = std::max(sp.min_spp, sp.step);
    uint32_t batch = (uint32_t)std::min<size_t>({(size_t)tile_count, ((size_t)256 << 20) / (64u * px_bytes), ((size_t)1 << 28) / (64u * (size_t)widest + TR_BLOCK)});
    if (batch == 0u) { set_error("Adaptive sampler: min_spp / max_spp too large for one tile's state"); return TRAY_E_UNSUPPORTED; }
    const size_t need = (size_t)batch * 64u * px_bytes;
    if (need > s->smp_bytes) {
        if (s->d_smp) { HIP_CHECK(hipStreamSynchronize(stream)); (void)hipFree(s->d_smp); s->d_smp = nullptr; s->smp_bytes = 0; }
        HIP_CHECK(hipMalloc(&s->d_smp, need));
        s->smp_bytes = need;
    }
    uint32_t* const px_state = static_cast<uint32_t*>(s->d_smp);
    float* const px_avg = reinterpret_cast<float*>(px_state + (size_t)batch * 64u);
    float* const px_lum = px_avg + (size_t)batch * 64u;
    if (!s->accumulate) HIP_CHECK(hipEventRecord(s->ev0, stream));
    uint32_t launches = 0;
    for (uint32_t item0 = 0; item0 < tile_count; item0 += batch) {
        const uint32_t n_items = std::min(batch, tile_count - item0), n_px = n_items * 64u;
        if (sp.kind == TRAY_SAMPLER_ADAPTIVE) HIP_CHECK(hipMemsetAsync(s->d_smp, 0, (size_t)batch * 64u * 8u, stream));   // states and averages
        for (uint32_t j = 0; j < rounds; ++j) {
            tr_rules::sampler_round(sp, j, smp_end ? smp_end - smp_begin : 0u);
            const uint32_t group = tr_rules::sampler_group(sp.count, SP_GROUP_MAX);
            const dim3 grid((n_items + group - 1u) / group), block(TR_BLOCK);
            const int anim = anim_debug(s);
            const bool lean = sampler_lean(s->feat, s->dev.integrator);
            if (sp.kind == TRAY_SAMPLER_LOW_DISCREPANCY && smp_end)
                tr_ranges::sampler_pass(anim, lean, grid, block, s->stack_bytes, stream, s->dev, tiles, item0, n_items, chunk, chunk_stride, kf, sp, px_state, px_lum,
                                        rgbw_dev, s->d_stats, group, smp_begin);
            else select_sampler_pass(anim, lean, [&](auto kernel) {
                hipLaunchKernelGGL(kernel, grid, block, s->stack_bytes, stream, s->dev, tiles, item0, n_items, chunk, chunk_stride, kf, sp, px_state, px_lum, rgbw_dev, s->d_stats, group);
            });
            ++launches;
            if (sp.kind == TRAY_SAMPLER_ADAPTIVE) {
                hipLaunchKernelGGL(k_sampler_decide, dim3((n_px + TR_BLOCK - 1) / TR_BLOCK), block, 0, stream, n_px, sp, px_state, px_avg, px_lum);
                ++launches;
            }
        }
    }
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(s->ev1, stream));
    s->timing_valid = true;
    s->launches = launches;
    return TRAY_OK;
}

// s->launch_dev, what the kernels of a render call get after launch_buffers_plan.h's prepare: `dev` with the cache, or the table in its place
static void fill_launch_dev(TrayDeviceScene* s) {
    const LaunchBuffers& b = s->lb;
    const bool table = b.st.last_used_table;
    DevScene& d = s->launch_dev;
    d = s->dev;
    d.xf_cache = b.xf_cache; d.xf_cache_lanes = b.st.cache_lanes;
    if (table) { d.xf_tab = b.d_xf_table; d.xf_tab_stride = b.st.table_stride; }
    if (table && s->wavefront) {   // the stage kernels index the table by the path's time index; the tile kernel keeps its cache columns and fills them from it
        d.xf_cache = b.d_xf_table; d.xf_table = 1u; d.xf_aos = 1u; d.xf_stride = b.st.table_stride;
    }
}

static int launch_tiles(TrayDeviceScene* s, const uint2* tiles, uint32_t tile_count, uint32_t chunk, uint32_t chunk_stride,
                        uint32_t spp, uint64_t seed, float* rgbw_dev, void* stream_, uint32_t smp_begin, uint32_t smp_end) {
    if (s->sampler_kind == TRAY_SAMPLER_LOW_DISCREPANCY && (spp == 0 || (spp & (spp - 1)) != 0)) {
        set_error("spp must be a power of two (LowDiscrepancy sampler, ld.rs:22-25); use tray_round_spp"); return TRAY_E_INVALID;
    }
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (s->broken) { set_error("this device scene is unusable: a tray_scene_update_frame on it failed"); return TRAY_E_INVALID; }
    HIP_CHECK(hipSetDevice(s->device));
    s->timing_valid = false;
    s->empty_launch = false;
    // (an empty queue is a valid work item -- a GPU's shard of a small frame dealt to many GPUs: tray_last_timing then reports zeros
    // instead of "no launch recorded", which made tray_multi_timing fail for 48 tiles on 8 devices: found by tests/test_multi_stub.py)
    if (tile_count == 0) { std::fprintf(stderr, "Warning: This block queue is empty!\n"); s->empty_launch = true; return TRAY_OK; }   // block_queue.rs:42-44
    HIP_CHECK(hipMemsetAsync(s->d_counter, 0, sizeof(uint32_t), stream));
    if (!s->accumulate) {   // (tray_render_noise_target_device clears them once for all its launches)
        HIP_CHECK(hipMemsetAsync(s->d_stats, 0, WF_STAT_SLOTS * sizeof(DevStats), stream));
        HIP_CHECK(hipMemsetAsync(s->d_retraced, 0, sizeof(uint32_t), stream));
    }
    const uint32_t kf = tr_rules::frame_key(seed, s->dev.frame);
    tr_rules::whole_frame_range(spp, smp_begin, smp_end);
    const uint32_t n_smp = tr_rules::range_samples(spp, smp_begin, smp_end);
    if (s->sampler_kind != TRAY_SAMPLER_LOW_DISCREPANCY || s->deforming) return launch_sampler(s, tiles, tile_count, chunk, chunk_stride, spp, kf, rgbw_dev, stream, smp_begin, smp_end);
    s->last_was_wavefront = false;
    const bool had_pool = s->lb.st.pool;
    {
        const auto t0 = std::chrono::steady_clock::now();
        LbOps lb_ops{s, stream};
        const int rc = tr_lbplan::prepare(lb_ops, s->lb.st, lb_facts(s), (uint64_t)tile_count * 64u * n_smp);
        if (getenv("TRAYHIP_STATS")) fprintf(stderr, "[trayhip] launch buffers prepared in %.1f ms (table %s, %u of %u records per index in use; pool %s: %u slots)\n",
                                             std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), s->lb.st.last_used_table ? "on" : "off",
                                             s->lb.st.table_stride, s->lb.st.table_cap, had_pool ? "kept" : "allocated", s->lb.st.pool_slots);
        if (rc != TRAY_OK) return rc;
        fill_launch_dev(s);
    }
    if (s->wavefront) {
        const auto t0 = std::chrono::steady_clock::now();
        const int rc = launch_wavefront(s, tiles, tile_count, chunk, chunk_stride, spp, kf, rgbw_dev, stream, smp_begin, smp_end);
        if (getenv("TRAYHIP_STATS")) fprintf(stderr, "[trayhip] wavefront launch enqueued in %.1f ms (pool %s: %u slots)\n",
                                             std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(), had_pool ? "kept" : "allocated", s->lb.st.pool_slots);
        return rc;
    }
    const uint32_t levels = tr_rules::tile_levels(tile_count, (uint32_t)s->n_blocks, n_smp);   // items per tile: progressive slices
    int blocks = (int)std::min<uint64_t>((uint64_t)s->n_blocks, (uint64_t)tile_count * levels);
#ifdef TR_SAMPLE_DUMP
    void* dump_buf = nullptr;
    const size_t dump_bytes = (size_t)s->dev.width * s->dev.height * spp * 8 * sizeof(float);
    if (getenv("TRAYHIP_SAMPLE_DUMP")) {
        HIP_CHECK(hipMalloc(&dump_buf, dump_bytes));
        HIP_CHECK(hipMemset(dump_buf, 0, dump_bytes));
    }
    s->launch_dev.sample_dump = static_cast<float4*>(dump_buf);
#endif
    if (!s->accumulate) HIP_CHECK(hipEventRecord(s->ev0, stream));
    const bool whitted = s->dev.integrator == TRAY_INTEGRATOR_WHITTED;
    const auto launch = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(blocks), dim3(TR_BLOCK), s->stack_bytes, stream, s->launch_dev, tiles, tile_count, chunk, chunk_stride, spp, kf, levels, rgbw_dev, s->d_counter, s->d_stats);
    };
    if (smp_end) tr_ranges::path_tiles(s->animated ? 1 : 0, s->feat, whitted, s->light_filter, dim3(blocks), dim3(TR_BLOCK), s->stack_bytes, stream,
                                       s->launch_dev, tiles, tile_count, chunk, chunk_stride, spp, kf, levels, rgbw_dev, s->d_counter, s->d_stats, smp_begin, smp_end);
    else if (runs_lean_tiles(s)) tr_tiles::path_tiles(s->feat, s->light_filter, dim3(blocks), dim3(TR_BLOCK), s->stack_bytes, stream, s->launch_dev, tiles, tile_count,
                                                      chunk, chunk_stride, spp, kf, levels, rgbw_dev, s->d_counter, s->d_stats);
    else if (s->animated) select_path_tiles<1>(s->feat, whitted, s->light_filter, launch);
    else select_path_tiles<0>(s->feat, whitted, s->light_filter, launch);
    if (getenv("TRAYHIP_STATS")) fprintf(stderr, "[trayhip] tile launch: %s kernel\n", smp_end ? "sample-range (libtrayhip_ranges.so)" : runs_lean_tiles(s) ? "lean (libtrayhip_tiles.so)" : "base (libtrayhip.so)");
    HIP_CHECK(hipGetLastError());
    HIP_CHECK(hipEventRecord(s->ev1, stream));
    s->timing_valid = true;
    s->launches = 1;
#ifdef TR_SAMPLE_DUMP   // instrumented builds only: TRAYHIP_SAMPLE_DUMP=<file> receives width x height x spp records of two float4 (radiance, vertices | final throughput, bounce) of the launch
    if (dump_buf) {
        HIP_CHECK(hipStreamSynchronize(stream));
        std::vector<float> host(dump_bytes / sizeof(float));
        HIP_CHECK(hipMemcpy(host.data(), dump_buf, dump_bytes, hipMemcpyDeviceToHost));
        (void)hipFree(dump_buf);
        if (FILE* fp = std::fopen(getenv("TRAYHIP_SAMPLE_DUMP"), "wb")) { std::fwrite(host.data(), 1, dump_bytes, fp); std::fclose(fp); }
    }
#endif
    return TRAY_OK;
}

int tray_render_tiles(TrayDeviceScene* s, uint32_t tile_start, uint32_t tile_count, uint32_t spp, uint64_t seed, float* rgbw_host) {
    if (!s || !rgbw_host) { set_error("tray_render_tiles: null argument"); return TRAY_E_INVALID; }
    HIP_CHECK(hipSetDevice(s->device));
    size_t n = (size_t)s->dev.width * s->dev.height * 4;
    float* d = nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    auto ms = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    HIP_CHECK(hipMalloc(&d, n * sizeof(float)));
    int rc = TRAY_OK;
    hipError_t e = hipMemset(d, 0, n * sizeof(float));
    double t_alloc = ms(), t_enq = 0.0, t_copy = 0.0;
    if (e == hipSuccess) {
        rc = tray_render_tiles_device(s, tile_start, tile_count, spp, seed, d, nullptr);
        t_enq = ms();
        if (rc == TRAY_OK) {
            std::vector<float> tmp(n);
            e = hipMemcpy(tmp.data(), d, n * sizeof(float), hipMemcpyDeviceToHost);
            t_copy = ms();
            if (e == hipSuccess)
                for (size_t i = 0; i < n; ++i) rgbw_host[i] += tmp[i];
        }
    }
    (void)hipFree(d);
    if (getenv("TRAYHIP_STATS")) fprintf(stderr, "[trayhip] tray_render_tiles: film buffer %.1f ms, enqueue %.1f, kernels + copy %.1f, add + free %.1f\n", t_alloc, t_enq - t_alloc, t_copy - t_enq, ms() - t_copy);
    if (e != hipSuccess) { set_error(std::string("tray_render_tiles: ") + hipGetErrorString(e)); return TRAY_E_DEVICE; }
    return rc;
}

// ---- several GPUs of this process: shard + RCCL sum-reduce inside the library ----------------------------------------------
namespace {
struct Rccl {   // the six entry points, resolved from librccl.so on first use
    void* lib = nullptr;
    int (*CommInitAll)(void**, int, const int*) = nullptr;
    int (*CommDestroy)(void*) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Reduce)(const void*, void*, size_t, int, int, int, void*, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
    bool load(std::string& err) {
        if (lib) return true;
        for (const char* name : {"librccl.so", "librccl.so.1", "/opt/rocm/lib/librccl.so"}) {
            lib = dlopen(name, RTLD_NOW | RTLD_LOCAL);
            if (lib) break;
        }
        if (!lib) { err = std::string("librccl.so could not be loaded: ") + dlerror(); return false; }
        CommInitAll = reinterpret_cast<decltype(CommInitAll)>(dlsym(lib, "ncclCommInitAll"));
        CommDestroy = reinterpret_cast<decltype(CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
        GroupStart = reinterpret_cast<decltype(GroupStart)>(dlsym(lib, "ncclGroupStart"));
        GroupEnd = reinterpret_cast<decltype(GroupEnd)>(dlsym(lib, "ncclGroupEnd"));
        Reduce = reinterpret_cast<decltype(Reduce)>(dlsym(lib, "ncclReduce"));
        GetErrorString = reinterpret_cast<decltype(GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
        if (!CommInitAll || !CommDestroy || !GroupStart || !GroupEnd || !Reduce || !GetErrorString) { err = "librccl.so lacks an expected entry point"; lib = nullptr; return false; }
        return true;
    }
};
Rccl g_rccl;
std::mutex g_rccl_mutex;
}  // namespace

struct TrayMultiScene {
    int n_dev = 0;
    std::vector<int> dev_ids;
    std::vector<TrayDeviceScene*> scenes;
    std::vector<float*> films;          // one full-frame RGBW buffer per device
    std::vector<hipStream_t> streams;
    std::vector<void*> comms;           // ncclComm_t
    size_t n_floats = 0;
    int partition = TRAY_PARTITION_TILES;   // tray_multi_set_partition
    float reduce_ms = 0.0f;
    hipEvent_t r0 = nullptr, r1 = nullptr;   // around the reduce, on the first device's stream
};

void tray_multi_destroy(TrayMultiScene* m) {
    if (!m) return;
    int current = 0;
    const bool have_current = hipGetDevice(&current) == hipSuccess;   // the caller's current device is left as it was
    for (int d = 0; d < (int)m->scenes.size(); ++d) {
        (void)hipSetDevice(m->dev_ids[d]);
        if (d < (int)m->comms.size() && m->comms[d] && g_rccl.CommDestroy) (void)g_rccl.CommDestroy(m->comms[d]);
        if (d < (int)m->films.size() && m->films[d]) (void)hipFree(m->films[d]);
        if (d < (int)m->streams.size() && m->streams[d]) (void)hipStreamDestroy(m->streams[d]);
        if (d == 0) { if (m->r0) (void)hipEventDestroy(m->r0); if (m->r1) (void)hipEventDestroy(m->r1); }
        tray_scene_destroy(m->scenes[d]);
    }
    if (have_current) (void)hipSetDevice(current);
    delete m;
}

int tray_multi_create(const TrayFlatScene* f, int n_dev, const int* dev_ids, TrayMultiScene** out) {
    if (!f || !out || !dev_ids || n_dev < 1) { set_error("tray_multi_create: null argument or no device"); return TRAY_E_INVALID; }
    *out = nullptr;
    int have = 0;
    HIP_CHECK(hipGetDeviceCount(&have));
    for (int d = 0; d < n_dev; ++d) {
        if (dev_ids[d] < 0 || dev_ids[d] >= have) { set_error("tray_multi_create: no such HIP device " + std::to_string(dev_ids[d])); return TRAY_E_INVALID; }
        for (int e = 0; e < d; ++e) if (dev_ids[e] == dev_ids[d]) { set_error("tray_multi_create: a device is listed twice"); return TRAY_E_INVALID; }
    }
    {
        std::lock_guard<std::mutex> lock(g_rccl_mutex);
        std::string err;
        if (!g_rccl.load(err)) { set_error("tray_multi_create: " + err); return TRAY_E_UNSUPPORTED; }
    }
    TrayMultiScene* m = new TrayMultiScene();
    m->n_dev = n_dev;
    m->dev_ids.assign(dev_ids, dev_ids + n_dev);
    m->n_floats = (size_t)f->film.width * f->film.height * 4;
    const int before = g_device;
    int rc = TRAY_OK;
    for (int d = 0; d < n_dev && rc == TRAY_OK; ++d) {
        rc = tray_init(dev_ids[d]);
        TrayDeviceScene* s = nullptr;
        if (rc == TRAY_OK) rc = tray_scene_create(f, &s);
        if (rc != TRAY_OK) break;
        m->scenes.push_back(s);
        float* film = nullptr;
        hipStream_t st = nullptr;
        if (hipMalloc(&film, m->n_floats * sizeof(float)) != hipSuccess || hipStreamCreate(&st) != hipSuccess) { set_error("tray_multi_create: film / stream allocation failed"); rc = TRAY_E_NOMEM; }
        m->films.push_back(film); m->streams.push_back(st);
    }
    if (rc == TRAY_OK) {
        m->comms.assign(n_dev, nullptr);
        const int nr = g_rccl.CommInitAll(m->comms.data(), n_dev, dev_ids);
        if (nr != 0) { set_error(std::string("ncclCommInitAll failed: ") + g_rccl.GetErrorString(nr)); rc = TRAY_E_DEVICE; }
    }
    if (rc == TRAY_OK) {
        (void)hipSetDevice(dev_ids[0]);
        if (hipEventCreate(&m->r0) != hipSuccess || hipEventCreate(&m->r1) != hipSuccess) { set_error("hipEventCreate failed"); rc = TRAY_E_DEVICE; }
    }
    (void)tray_init(before);
    if (rc != TRAY_OK) { tray_multi_destroy(m); return rc; }
    *out = m;
    return TRAY_OK;
}

// The same scene at another frame on every device (tray_scene_update_frame); communicators, films and streams stay.
int tray_multi_set_sampler(TrayMultiScene* m, uint32_t kind, uint32_t min_spp, uint32_t max_spp) {
    if (!m) { set_error("tray_multi_set_sampler: null argument"); return TRAY_E_INVALID; }
    for (TrayDeviceScene* s : m->scenes) {
        const int rc = tray_scene_set_sampler(s, kind, min_spp, max_spp);
        if (rc != TRAY_OK) return rc;
    }
    return TRAY_OK;
}

int tray_multi_set_partition(TrayMultiScene* m, int partition) {
    if (!m) { set_error("tray_multi_set_partition: null argument"); return TRAY_E_INVALID; }
    if (partition != TRAY_PARTITION_TILES && partition != TRAY_PARTITION_SAMPLES) { set_error("tray_multi_set_partition: unknown partition " + std::to_string(partition)); return TRAY_E_INVALID; }
    m->partition = partition;
    return TRAY_OK;
}

int tray_multi_update_frame(TrayMultiScene* m, const TrayFlatScene* f) {
    if (!m || !f) { set_error("tray_multi_update_frame: null argument"); return TRAY_E_INVALID; }
    int current = 0;
    const bool have_current = hipGetDevice(&current) == hipSuccess;
    int rc = TRAY_OK;
    for (int d = 0; d < m->n_dev && rc == TRAY_OK; ++d) rc = tray_scene_update_frame(m->scenes[d], f);
    if (have_current) (void)hipSetDevice(current);
    return rc;
}

struct CurrentDeviceGuard {   // the multi-device entry points leave the caller's current HIP device as they found it
    int dev = 0;
    bool ok = false;
    CurrentDeviceGuard() { ok = hipGetDevice(&dev) == hipSuccess; }
    ~CurrentDeviceGuard() { if (ok) (void)hipSetDevice(dev); }
};

int tray_render_frame_multi(TrayMultiScene* m, uint32_t spp, uint64_t seed, float* rgbw_host) {
    if (!m || !rgbw_host) { set_error("tray_render_frame_multi: null argument"); return TRAY_E_INVALID; }
    const bool by_samples = m->partition == TRAY_PARTITION_SAMPLES;
    if (by_samples) {   // (refused before any device starts: a range of Uniform / Adaptive has no meaning)
        if (spp == 0 || (spp & (spp - 1)) != 0) { set_error("spp must be a power of two (LowDiscrepancy sampler, ld.rs:22-25); use tray_round_spp"); return TRAY_E_INVALID; }
        for (TrayDeviceScene* s : m->scenes)
            if (s->sampler_kind != TRAY_SAMPLER_LOW_DISCREPANCY) { set_error("tray_render_frame_multi: the samples partition needs the LowDiscrepancy sampler"); return TRAY_E_UNSUPPORTED; }
    }
    CurrentDeviceGuard keep_current;
    // one host thread per device: the wavefront schedule polls its stream, and the launches of different devices must overlap
    std::vector<int> rcs(m->n_dev, TRAY_OK);
    std::vector<std::string> errs(m->n_dev);
    std::vector<std::thread> workers;
    for (int d = 0; d < m->n_dev; ++d)
        workers.emplace_back([&, d] {
            if (hipSetDevice(m->dev_ids[d]) != hipSuccess || hipMemsetAsync(m->films[d], 0, m->n_floats * sizeof(float), m->streams[d]) != hipSuccess) {
                rcs[d] = TRAY_E_DEVICE; errs[d] = "hipSetDevice / hipMemsetAsync failed"; return;
            }
            if (by_samples) {   // every tile, device d's range of the samples (exec/distrib/master.rs:91-93 deals blocks; the film is a sum either way)
                uint32_t b = 0u, e = 0u;
                (void)tray_multi_shard_samples(spp, (uint32_t)d, (uint32_t)m->n_dev, &b, &e);
                rcs[d] = b < e ? tray_render_samples_device(m->scenes[d], 0u, 0u, spp, b, e, seed, m->films[d], m->streams[d])
                               : launch_tiles(m->scenes[d], m->scenes[d]->d_tiles, 0, 1, 1, spp, seed, m->films[d], m->streams[d]);   // (an empty range: no launch, the film joins the reduce as zeros)
            } else {
                rcs[d] = tray_render_shard_device(m->scenes[d], (uint32_t)d, (uint32_t)m->n_dev, 16u, spp, seed, m->films[d], m->streams[d]);
            }
            if (rcs[d] != TRAY_OK) errs[d] = tray_last_error();
        });
    for (std::thread& w : workers) w.join();
    for (int d = 0; d < m->n_dev; ++d)
        if (rcs[d] != TRAY_OK) { set_error("tray_render_frame_multi: device " + std::to_string(m->dev_ids[d]) + ": " + errs[d]); return rcs[d]; }
    // film::Image::add_blocks on the master == one sum-reduce onto the first device (in place on the root). Every device's shard is
    // finished before the reduce is timed, so reduce_ms is the collective alone, not the wait for the slowest shard
    for (int d = 0; d < m->n_dev; ++d) { HIP_CHECK(hipSetDevice(m->dev_ids[d])); HIP_CHECK(hipStreamSynchronize(m->streams[d])); }
    HIP_CHECK(hipSetDevice(m->dev_ids[0]));
    HIP_CHECK(hipEventRecord(m->r0, m->streams[0]));
    int nr = g_rccl.GroupStart();
    for (int d = 0; d < m->n_dev && nr == 0; ++d) {
        (void)hipSetDevice(m->dev_ids[d]);
        nr = g_rccl.Reduce(m->films[d], m->films[d], m->n_floats, /*ncclFloat*/ 7, /*ncclSum*/ 0, /*root*/ 0, m->comms[d], m->streams[d]);
    }
    const int ne = g_rccl.GroupEnd();
    if (nr == 0) nr = ne;
    if (nr != 0) { set_error(std::string("ncclReduce failed: ") + g_rccl.GetErrorString(nr)); return TRAY_E_DEVICE; }
    HIP_CHECK(hipSetDevice(m->dev_ids[0]));
    HIP_CHECK(hipEventRecord(m->r1, m->streams[0]));
    for (int d = 0; d < m->n_dev; ++d) { HIP_CHECK(hipSetDevice(m->dev_ids[d])); HIP_CHECK(hipStreamSynchronize(m->streams[d])); }
    HIP_CHECK(hipSetDevice(m->dev_ids[0]));
    HIP_CHECK(hipEventElapsedTime(&m->reduce_ms, m->r0, m->r1));
    std::vector<float> tmp(m->n_floats);
    HIP_CHECK(hipMemcpy(tmp.data(), m->films[0], m->n_floats * sizeof(float), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < m->n_floats; ++i) rgbw_host[i] += tmp[i];
    return TRAY_OK;
}

int tray_scene_set_transform_table(TrayDeviceScene* s, int mode) {
    if (!s) { set_error("tray_scene_set_transform_table: null argument"); return TRAY_E_INVALID; }
    if (mode < -1 || mode > 1) { set_error("tray_scene_set_transform_table: mode is -1 (by the launch's sample count), 0 (never) or 1 (always)"); return TRAY_E_INVALID; }
    s->xf_table_req = mode;
    return TRAY_OK;
}
int tray_multi_set_transform_table(TrayMultiScene* m, int mode) {
    if (!m) { set_error("tray_multi_set_transform_table: null argument"); return TRAY_E_INVALID; }
    for (TrayDeviceScene* s : m->scenes) {
        const int rc = tray_scene_set_transform_table(s, mode);
        if (rc != TRAY_OK) return rc;
    }
    return TRAY_OK;
}
int tray_debug_transform_table(TrayDeviceScene* s, uint32_t n, uint32_t* n_differ) {
    if (!s || !n_differ) { set_error("tray_debug_transform_table: null argument"); return TRAY_E_INVALID; }
    *n_differ = 0;
    if (!s->lb.st.table || !s->lb.st.table_built) { set_error("tray_debug_transform_table: this frame has no transform table (no launch wanted one yet)"); return TRAY_E_INVALID; }
    HIP_CHECK(hipSetDevice(s->device));
    uint32_t* d_bad = nullptr;
    HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&d_bad), sizeof(uint32_t)));
    hipError_t e = hipMemset(d_bad, 0, sizeof(uint32_t));
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_xf_table_check, dim3((n + TR_BLOCK - 1) / TR_BLOCK), dim3(TR_BLOCK), 0, nullptr, s->dev, s->lb.d_xf_table, s->lb.st.table_stride, n, d_bad);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(n_differ, d_bad, sizeof(uint32_t), hipMemcpyDeviceToHost);
    (void)hipFree(d_bad);
    if (e != hipSuccess) { set_error(std::string("tray_debug_transform_table: ") + hipGetErrorString(e)); return TRAY_E_DEVICE; }
    return TRAY_OK;
}
int tray_scene_set_wavefront(TrayDeviceScene* s, uint32_t pool_slots, uint32_t views, uint32_t slices) {
    if (!s) { set_error("tray_scene_set_wavefront: null argument"); return TRAY_E_INVALID; }
    if (s->broken) { set_error("tray_scene_set_wavefront: the handle is only good for tray_scene_destroy after a failed frame update"); return TRAY_E_INVALID; }
    if (views > (uint32_t)WF_PIPES_MAX) { set_error("tray_scene_set_wavefront: at most " + std::to_string(WF_PIPES_MAX) + " views"); return TRAY_E_INVALID; }
    if (slices > WF_MAX_SLICES || (slices & (slices - 1u)) != 0u) { set_error("tray_scene_set_wavefront: slices per tile must be 0 or a power of two up to " + std::to_string(WF_MAX_SLICES)); return TRAY_E_INVALID; }
    const bool pool_goes = tr_lbplan::wish_changed(s->lb.st, s->n_tiles, s->wf_req_slots, pool_slots);
    s->wf_req_slots = pool_slots; s->wf_req_views = views; s->wf_req_slices = slices;
    if (pool_goes) {   // another pool size: the buffers go, the next render call allocates them anew
        HIP_CHECK(hipSetDevice(s->device));
        HIP_CHECK(hipDeviceSynchronize());
        LbOps ops{s};
        tr_lbplan::drop_pool(ops, s->lb.st);
    }
    return TRAY_OK;
}
int tray_multi_set_wavefront(TrayMultiScene* m, uint32_t pool_slots, uint32_t views, uint32_t slices) {
    if (!m) { set_error("tray_multi_set_wavefront: null argument"); return TRAY_E_INVALID; }
    for (TrayDeviceScene* s : m->scenes) {
        const int rc = tray_scene_set_wavefront(s, pool_slots, views, slices);
        if (rc != TRAY_OK) return rc;
    }
    return TRAY_OK;
}
int tray_last_schedule(TrayDeviceScene* s, TrayScheduleInfo* out) {
    if (!s || !out) { set_error("tray_last_schedule: null argument"); return TRAY_E_INVALID; }
    std::memset(out, 0, sizeof *out);
    out->wavefront = s->wavefront ? 1u : 0u;
    out->launched_wavefront = s->last_was_wavefront ? 1u : 0u;
    const tr_lbplan::State& st = s->lb.st;   // (a part that does not exist has no slots, bytes or records)
    out->pool_slots = st.pool_slots; out->chunks = s->lb.wf.n_chunks;
    out->views = s->last_was_wavefront ? s->last_views : 0u; out->slices = s->last_was_wavefront ? s->last_slices : 0u;
    out->pool_bytes = tr_lbplan::pool_bytes(st.pool_slots);
    out->schedule_bytes = st.pool_slots * tr_lbplan::schedule_bytes_per_slot();
    out->xf_cache_bytes = st.cache_bytes;
    out->n_moving = s->dev.n_moving;
    out->tile_workgroups = (uint32_t)s->n_blocks;
    out->transform_table = st.last_used_table ? 1u : 0u;
    out->binned_stages = (s->last_was_wavefront && WF_FOLD_C) ? s->wf_bin_stages : 0u;
    out->xf_table_bytes = tr_lbplan::table_bytes(st.table_cap);   // (the buffer: sized for what any frame of the sequence can move)
    return TRAY_OK;
}

int tray_last_timing(TrayDeviceScene* s, TrayKernelTiming* t);
int tray_multi_timing(TrayMultiScene* m, TrayKernelTiming* per_device, float* reduce_ms) {
    if (!m || !per_device) { set_error("tray_multi_timing: null argument"); return TRAY_E_INVALID; }
    CurrentDeviceGuard keep_current;   // (tray_last_timing makes each scene's device current: found by tests/test_multi_stub.py)
    for (int d = 0; d < m->n_dev; ++d) {
        const int rc = tray_last_timing(m->scenes[d], per_device + d);
        if (rc != TRAY_OK) return rc;
    }
    if (reduce_ms) *reduce_ms = m->reduce_ms;
    return TRAY_OK;
}

int tray_last_timing(TrayDeviceScene* s, TrayKernelTiming* t) {
    if (!s || !t) { set_error("tray_last_timing: null argument"); return TRAY_E_INVALID; }
    std::memset(t, 0, sizeof *t);
    if (s->empty_launch) return TRAY_OK;
    if (!s->timing_valid) { set_error("tray_last_timing: no launch recorded"); return TRAY_E_INVALID; }
    HIP_CHECK(hipSetDevice(s->device));
    HIP_CHECK(hipEventSynchronize(s->ev1));
    HIP_CHECK(hipEventElapsedTime(&t->render_ms, s->ev0, s->ev1));
    std::vector<DevStats> all(WF_STAT_SLOTS);
    HIP_CHECK(hipMemcpy(all.data(), s->d_stats, all.size() * sizeof(DevStats), hipMemcpyDeviceToHost));
    DevStats st{};
    for (const DevStats& a : all) {
        st.samples += a.samples; st.vertices += a.vertices; st.rays += a.rays;
        for (int k = 0; k < 18; ++k) st.trav[k] += a.trav[k];
    }
#ifdef TR_STAGE_CLOCKS
    if (getenv("TRAYHIP_STATS") && st.trav[0]) {
        double tot = 0;
        for (int k = 0; k < 7; ++k) tot += (double)st.trav[k];
        const char* names[7] = {"trace A", "trace B", "trace C", "vertex_begin", "queries", "vertex_end", "regen+film"};
        for (int k = 0; k < 7; ++k) fprintf(stderr, "[trayhip] %-12s %5.1f %% of wave cycles\n", names[k], 100.0 * (double)st.trav[k] / tot);
        const char* parts[3] = {"sample head / light setup", "eval + pdf site", "epilogue of the query kind"};
        for (int k = 0; k < 3; ++k) fprintf(stderr, "[trayhip]   queries: %-28s %5.1f %% of wave cycles\n", parts[k], 100.0 * (double)st.trav[8 + k] / tot);
    }
#elif defined(WF_TRACE_CLOCKS)
    if (getenv("TRAYHIP_STATS") && st.rays)
        for (int g = 0; g < 3; ++g) {
            const unsigned long long* t = st.trav + g * 6;
            double tot = 0;
            for (int k = 0; k < 5; ++k) tot += (double)t[k];
            if (tot > 0) fprintf(stderr, "[trayhip] trace %c wave cycles: refill %.1f %%  node phase %.1f %%  leaf phase %.1f %%  pop phase %.1f %%  result write %.1f %%  (%.3e clock64 ticks in all waves)\n", "ABC"[g],
                                 100 * t[0] / tot, 100 * t[1] / tot, 100 * t[2] / tot, 100 * t[3] / tot, 100 * t[4] / tot, tot);
        }
#else
    if (getenv("TRAYHIP_STATS") && st.rays)
        for (int g = 0; g < 3; ++g) {
            const unsigned long long* t = st.trav + g * 6;
            if (!t[5]) continue;
            fprintf(stderr, "[trayhip] stage %c: %llu rays; per ray: node steps %.2f  single-node visits %.2f  two-child expansions %.2f  instance entries %.2f  triangle tests %.2f\n",
                    "ABC"[g], t[5], (double)t[0] / t[5], (double)t[1] / t[5], (double)t[2] / t[5], (double)t[3] / t[5], (double)t[4] / t[5]);
        }
#endif
    uint32_t retraced = 0;
    HIP_CHECK(hipMemcpy(&retraced, s->d_retraced, sizeof retraced, hipMemcpyDeviceToHost));
    t->launches = s->launches;
    t->samples = st.samples; t->vertices = st.vertices; t->rays = st.rays; t->retraced = retraced;
    return TRAY_OK;
}

int tray_debug_intersect(TrayDeviceScene* s, uint32_t n, const TrayRay* rays, TrayHit* hits) {
    if (!s || !rays || !hits) { set_error("tray_debug_intersect: null argument"); return TRAY_E_INVALID; }
    if (n == 0) return TRAY_OK;
    HIP_CHECK(hipSetDevice(s->device));
    TrayRay* d_r = nullptr;
    TrayHit* d_h = nullptr;
    HIP_CHECK(hipMalloc(&d_r, n * sizeof(TrayRay)));
    hipError_t e = hipMalloc(&d_h, n * sizeof(TrayHit));
    if (e == hipSuccess) e = hipMemcpy(d_r, rays, n * sizeof(TrayRay), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        // ANIM = 2: debug grids are sized by the item count, not by the transform cache, so the spline stacks are evaluated at every use
        const int anim = anim_debug(s);
        if (anim == 3) hipLaunchKernelGGL(k_debug_intersect<3>, dim3((n + TR_BLOCK - 1) / TR_BLOCK), dim3(TR_BLOCK), s->stack_bytes, 0, s->dev, n, d_r, d_h);
        else if (anim == 2) hipLaunchKernelGGL(k_debug_intersect<2>, dim3((n + TR_BLOCK - 1) / TR_BLOCK), dim3(TR_BLOCK), s->stack_bytes, 0, s->dev, n, d_r, d_h);
        else hipLaunchKernelGGL(k_debug_intersect<0>, dim3((n + TR_BLOCK - 1) / TR_BLOCK), dim3(TR_BLOCK), s->stack_bytes, 0, s->dev, n, d_r, d_h);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(hits, d_h, n * sizeof(TrayHit), hipMemcpyDeviceToHost);
    (void)hipFree(d_r);
    (void)hipFree(d_h);
    if (e != hipSuccess) { set_error(std::string("tray_debug_intersect: ") + hipGetErrorString(e)); return TRAY_E_DEVICE; }
    return TRAY_OK;
}

int tray_debug_sample_radiance(TrayDeviceScene* s, uint32_t n, const uint32_t* px, const uint32_t* py, const uint32_t* si,
                               uint32_t spp, uint64_t seed, float* out) {
    if (!s || !px || !py || !si || !out) { set_error("tray_debug_sample_radiance: null argument"); return TRAY_E_INVALID; }
    if (spp == 0 || (spp & (spp - 1)) != 0) { set_error("spp must be a power of two"); return TRAY_E_INVALID; }
    if (n == 0) return TRAY_OK;
    for (uint32_t i = 0; i < n; ++i)
        if (px[i] >= s->dev.width || py[i] >= s->dev.height || si[i] >= spp) { set_error("tray_debug_sample_radiance: item out of range"); return TRAY_E_INVALID; }
    HIP_CHECK(hipSetDevice(s->device));
    uint32_t* d_in = nullptr;
    float* d_out = nullptr;
    HIP_CHECK(hipMalloc(&d_in, 3 * (size_t)n * sizeof(uint32_t)));
    hipError_t e = hipMalloc(&d_out, 8 * (size_t)n * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(d_in, px, n * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_in + n, py, n * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_in + 2 * (size_t)n, si, n * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        auto mix = [](uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; };
        uint32_t kf = mix((uint32_t)seed + 0x9E3779B9u);
        kf = mix(kf ^ (uint32_t)(seed >> 32));
        kf = mix(kf + s->dev.frame);
        const int anim = anim_debug(s);
        if (anim == 3)
            hipLaunchKernelGGL(k_debug_sample_radiance<3>, dim3((n + TR_BLOCK - 1) / TR_BLOCK), dim3(TR_BLOCK), s->stack_bytes, 0, s->dev, n, d_in, d_in + n, d_in + 2 * (size_t)n, spp, kf, d_out);
        else if (anim == 2)
            hipLaunchKernelGGL(k_debug_sample_radiance<2>, dim3((n + TR_BLOCK - 1) / TR_BLOCK), dim3(TR_BLOCK), s->stack_bytes, 0, s->dev, n, d_in, d_in + n, d_in + 2 * (size_t)n, spp, kf, d_out);
        else
            hipLaunchKernelGGL(k_debug_sample_radiance<0>, dim3((n + TR_BLOCK - 1) / TR_BLOCK), dim3(TR_BLOCK), s->stack_bytes, 0, s->dev, n, d_in, d_in + n, d_in + 2 * (size_t)n, spp, kf, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d_out, 8 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    if (e != hipSuccess) { set_error(std::string("tray_debug_sample_radiance: ") + hipGetErrorString(e)); return TRAY_E_DEVICE; }
    return TRAY_OK;
}

int tray_debug_first_hit(TrayDeviceScene* s, uint32_t n, const uint32_t* px, const uint32_t* py, const uint32_t* si, uint32_t spp, uint64_t seed, float* out) {
    if (!s || !px || !py || !si || !out) { set_error("tray_debug_first_hit: null argument"); return TRAY_E_INVALID; }
    if (spp == 0 || (spp & (spp - 1)) != 0) { set_error("spp must be a power of two"); return TRAY_E_INVALID; }
    if (n == 0) return TRAY_OK;
    for (uint32_t i = 0; i < n; ++i)
        if (px[i] >= s->dev.width || py[i] >= s->dev.height || si[i] >= spp) { set_error("tray_debug_first_hit: item out of range"); return TRAY_E_INVALID; }
    HIP_CHECK(hipSetDevice(s->device));
    uint32_t* d_in = nullptr;
    float* d_out = nullptr;
    HIP_CHECK(hipMalloc(&d_in, 3 * (size_t)n * sizeof(uint32_t)));
    hipError_t e = hipMalloc(&d_out, 12 * (size_t)n * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(d_in, px, n * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_in + n, py, n * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_in + 2 * (size_t)n, si, n * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        tr_firsthit::debug(anim_debug(s), s->stack_bytes, s->dev, n, d_in, d_in + n, d_in + 2 * (size_t)n, spp, tr_rules::frame_key(seed, s->dev.frame), d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d_out, 12 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    if (e != hipSuccess) { set_error(std::string("tray_debug_first_hit: ") + hipGetErrorString(e)); return TRAY_E_DEVICE; }
    return TRAY_OK;
}

int tray_debug_bsdf(TrayDeviceScene* s, uint32_t material_id, uint32_t flags, uint32_t n, const float* dirs, const float* u3, float* out) {
    if (!s || !dirs || !u3 || !out) { set_error("tray_debug_bsdf: null argument"); return TRAY_E_INVALID; }
    if (n == 0) return TRAY_OK;
    if (material_id >= s->n_materials) { set_error("tray_debug_bsdf: no such material"); return TRAY_E_INVALID; }
    HIP_CHECK(hipSetDevice(s->device));
    // private one-instance table carrying the requested material
    TrayInstance fake;
    std::memset(&fake, 0, sizeof fake);
    fake.material_id = material_id;
    TrayInstance* d_fake = nullptr;
    float *d_dirs = nullptr, *d_u = nullptr, *d_out = nullptr;
    HIP_CHECK(hipMalloc(&d_fake, sizeof fake));
    hipError_t e = hipMalloc(&d_dirs, 6 * (size_t)n * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&d_u, 3 * (size_t)n * sizeof(float));
    if (e == hipSuccess) e = hipMalloc(&d_out, 12 * (size_t)n * sizeof(float));
    if (e == hipSuccess) e = hipMemcpy(d_fake, &fake, sizeof fake, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_dirs, dirs, 6 * (size_t)n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_u, u3, 3 * (size_t)n * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        DevScene tmp = s->dev;
        tmp.instances = d_fake;
        hipLaunchKernelGGL(k_debug_bsdf, dim3((n + 63) / 64), dim3(64), 0, 0, tmp, flags, n, d_dirs, d_u, d_out);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(out, d_out, 12 * (size_t)n * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(d_fake); (void)hipFree(d_dirs); (void)hipFree(d_u); (void)hipFree(d_out);
    if (e != hipSuccess) { set_error(std::string("tray_debug_bsdf: ") + hipGetErrorString(e)); return TRAY_E_DEVICE; }
    return TRAY_OK;
}

}  // extern "C"
