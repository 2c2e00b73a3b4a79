// Host emulation of the sample-range launches (tray_render_samples_device): the entry points of emu_kernels.cpp for the tile kernel, the
// wavefront schedule and the sampler pass, with the range [smp_begin, smp_end) of the spp-sample LowDiscrepancy frame handed to the kernels
// as device_api.hip hands it (0 / 0, or [0, spp): the whole frame) and the launch rules (levels, slice_shift, rounds) applied to its n samples.
// Built by tests/test_sample_ranges_emu.py: the same device sources as libtrayemu.so, with the range arguments of libtrayhip_ranges.so's
// instantiations (TR_SAMPLE_RANGES; emu_kernels.cpp's own entry points pass none and render whole frames).
#define TR_SAMPLE_RANGES
#include "emu_kernels.cpp"

extern "C" {

// emu_render_tiles over a sample range (no shards)
int emu_render_tiles_range(const TrayFlatScene* f, const uint32_t* tiles_xy, uint32_t tile_count, uint32_t spp, uint32_t smp_begin, uint32_t smp_end,
                           uint64_t seed, float* rgbw, uint32_t blocks, int coop, int film_rows, unsigned long long* stats_out) {
    const uint32_t shard = 0u, n_shards = 0u, chunk_tiles = 1u;
    if (smp_begin == 0u && smp_end == spp) smp_end = 0u;   // (launch_tiles: the whole frame as a range is the whole-frame launch)
    const uint32_t n_smp = smp_end ? smp_end - smp_begin : spp;
    EmuScene e;
    make_scene(f, e);
    bool moving = f->camera.animated != 0;
    for (uint32_t t_ = 0; t_ < f->n_textures; ++t_) moving = moving || f->textures[t_].n_frames >= 2u;   // animated_image needs ray.time (tray_scene_create)
    for (uint32_t i = 0; i < f->n_instances; ++i) moving = moving || f->instances[i].animated != 0 || f->instances[i].emis_count >= 2;
    if (f->n_instances > TR_FLAT_MAX && !moving) return -4;   // the library runs the wavefront schedule for those
    uint32_t n_moving = 0;
    for (uint32_t i = 0; i < f->n_instances; ++i) if (f->instances[i].animated) ++n_moving;
    std::vector<uint32_t> moving_ids(std::max(n_moving, 1u), 0u);
    std::vector<float> xf_cache;
    if (moving && n_moving) {   // per-path transform cache, one column per thread of the grid (tray_scene_create)
        for (uint32_t i = 0; i < f->n_instances; ++i)
            if (f->instances[i].animated && f->instances[i].moving_slot < n_moving) moving_ids[f->instances[i].moving_slot] = i;
        xf_cache.assign((size_t)n_moving * TR_XF_WORDS * blocks * TR_BLOCK, 0.0f);
        e.d.xf_cache = xf_cache.data(); e.d.moving_ids = moving_ids.data(); e.d.n_moving = n_moving; e.d.xf_stride = n_moving; e.d.xf_cache_lanes = blocks * TR_BLOCK;
    }
    SparseXfTable table;   // TRAYHIP_EMU_XF_TABLE=1: the fill of the cache columns FROM THE TABLE (dev_geom.h: xf_cache_fill_wave, camera_ray) runs in the emulation
    if (moving && getenv("TRAYHIP_EMU_XF_TABLE") && atoi(getenv("TRAYHIP_EMU_XF_TABLE")) != 0) {
        if (!table.build(f, e.d.frame, moving_ids.data(), n_moving, tiles_xy, tile_count, spp, seed)) return -5;
        if (table.data) { e.d.moving_ids = moving_ids.data(); e.d.xf_tab = table.data; e.d.xf_tab_stride = table.stride; }
    }
    e.d.film_rows = (film_rows != 0 && film_rows_ok(f)) ? 1u : 0u;
    uint32_t stack_words = e.depth * TR_BLOCK;
    bool small_mesh = false;
    for (uint32_t m = 0; m < f->n_meshes; ++m) small_mesh = small_mesh || f->meshes[m].tri_count <= TR_COOP_MAX_TRIS;
    if (coop != 0 && small_mesh && f->n_instances <= TR_FLAT_MAX) { e.d.coop_offset = stack_words; stack_words += (TR_BLOCK / 64) * TR_COOP_WORDS; }
    if (e.d.film_rows) { e.d.win_offset = 0u; stack_words = std::max(stack_words, 4u * WIN_PLANE); }   // tray_scene_create: the film window over the stacks ...
    else { e.d.win_offset = stack_words; stack_words += 4u * WIN_PLANE; }                               // ... or in its own region
    std::vector<uint2> tiles(tile_count);
    for (uint32_t i = 0; i < tile_count; ++i) tiles[i] = make_uint2(tiles_xy[2 * i], tiles_xy[2 * i + 1]);
    // work-item mapping of launch_tiles: item w -> queue entry (w / chunk) * chunk_stride * chunk + (w % chunk), from tile_start on
    uint32_t tile_start = 0, work = tile_count, chunk = tile_count ? tile_count : 1u, chunk_stride = 1u;
    if (n_shards) {   // tray_render_shard_device
        const uint32_t n_chunks = (tile_count + chunk_tiles - 1) / chunk_tiles;
        const uint32_t my_chunks = shard < n_chunks ? (n_chunks - shard + n_shards - 1) / n_shards : 0;
        if (my_chunks == 0) { if (stats_out) stats_out[0] = stats_out[1] = stats_out[2] = stats_out[3] = 0; return 0; }
        const uint32_t last_chunk = shard + (my_chunks - 1) * n_shards;
        uint32_t tail = tile_count - last_chunk * chunk_tiles;
        if (tail > chunk_tiles) tail = chunk_tiles;
        tile_start = shard * chunk_tiles; work = (my_chunks - 1) * chunk_tiles + tail; chunk = chunk_tiles; chunk_stride = n_shards;
    }
    uint32_t counter = 0;
    DevStats stats;
    std::memset(&stats, 0, sizeof stats);
    const uint32_t kf = key_frame_host(seed, e.d.frame);
    const int feat = feature_set(e);
    uint32_t levels = 1u;   // launch_tiles' rule: tiles are cut into progressive sample slices when there are few of them per workgroup
    { const bool small = work < 12u * blocks; const uint32_t most = small ? 5u : 3u, least = small ? 64u : 256u; while (levels < most && (n_smp >> levels) >= least) ++levels; }
    if (const char* e_ = getenv("TRAYHIP_TILE_SLICES")) { levels = 1u; const uint32_t want = (uint32_t)std::max(1, atoi(e_)); while (levels < want && (n_smp >> levels) >= 1u) ++levels; }
    int rc;
    // tray_scene_create: the instantiation with mis_ray_filter for scenes with a sphere light or specular lobes
    bool light_filter = (feat & FEAT_SPEC) != 0;
    for (uint32_t l = 0; l < f->n_lights; ++l)
        if (f->instances[f->lights[l]].kind != TRAY_INST_POINT_EMITTER && f->instances[f->lights[l]].geom_type == TRAY_GEOM_SPHERE) light_filter = true;
#define EMU_TILES_L(A, F, L) launch_simt(blocks, TR_BLOCK, [&] { k_path_tiles<A, F, TRAY_INTEGRATOR_PATH, L>(e.d, tiles.data() + tile_start, work, chunk, chunk_stride, spp, kf, levels, rgbw, &counter, &stats, smp_begin, smp_end); }, (size_t)stack_words * 4)
#define EMU_TILES(F) rc = moving ? (light_filter ? EMU_TILES_L(1, F, true) : EMU_TILES_L(1, F, false)) : (light_filter ? EMU_TILES_L(0, F, true) : EMU_TILES_L(0, F, false))
#define EMU_WHITTED(A) launch_simt(blocks, TR_BLOCK, [&] { k_path_tiles<A, FEAT_ALL | FEAT_TEX, TRAY_INTEGRATOR_WHITTED>(e.d, tiles.data() + tile_start, work, chunk, chunk_stride, spp, kf, levels, rgbw, &counter, &stats, smp_begin, smp_end); }, (size_t)stack_words * 4)
    if (e.d.integrator == TRAY_INTEGRATOR_WHITTED) rc = moving ? EMU_WHITTED(1) : EMU_WHITTED(0);   // launch_tiles: one instantiation per ANIM
    else if (feat == FEAT_NONE) EMU_TILES(FEAT_NONE);
    else if (feat == FEAT_MERL) EMU_TILES(FEAT_MERL);
    else if (feat == FEAT_SPEC) EMU_TILES(FEAT_SPEC);
    else if (feat == (FEAT_MERL | FEAT_SPEC)) EMU_TILES(FEAT_MERL | FEAT_SPEC);
    else if (feat == (FEAT_ALL | FEAT_TEX)) EMU_TILES(FEAT_ALL | FEAT_TEX);
    else EMU_TILES(FEAT_ALL);
#undef EMU_TILES
#undef EMU_TILES_L
#undef EMU_WHITTED
    if (stats_out) { stats_out[0] = stats.samples; stats_out[1] = stats.vertices; stats_out[2] = stats.rays; stats_out[3] = (unsigned long long)feat; }
    return rc;
}

// emu_render_wavefront over a sample range (trace 0, the full LDS stack)
int emu_render_wavefront_range(const TrayFlatScene* f, const uint32_t* tiles_xy, uint32_t tile_count, uint32_t spp, uint32_t smp_begin, uint32_t smp_end,
                               uint64_t seed, float* rgbw, uint32_t n_chunks, uint32_t trace_blocks, unsigned long long* stats_out) {
    const int trace = 0;
    uint32_t lds_depth = 0u;
    if (smp_begin == 0u && smp_end == spp) smp_end = 0u;
    const uint32_t n_smp = smp_end ? smp_end - smp_begin : spp;
    EmuScene e;
    make_scene(f, e);
    bool moving = f->camera.animated != 0;
    for (uint32_t t_ = 0; t_ < f->n_textures; ++t_) moving = moving || f->textures[t_].n_frames >= 2u;   // animated_image needs ray.time (tray_scene_create)
    uint32_t n_moving = 0;
    for (uint32_t i = 0; i < f->n_instances; ++i) {
        moving = moving || f->instances[i].animated != 0 || f->instances[i].emis_count >= 2;
        if (f->instances[i].animated) ++n_moving;
    }
    e.d.film_rows = film_rows_ok(f) ? 1u : 0u;
    // launch_wavefront's rule: tiles are cut into slices of their samples while the pool has more chunks than work items (k_wf_advance)
    uint32_t slice_shift = 0u;
    while ((1u << (slice_shift + 1u)) <= 16u && ((uint64_t)tile_count << (slice_shift + 1u)) <= n_chunks && (n_smp >> (slice_shift + 1u)) >= 16u) ++slice_shift;
    if (const char* sl = getenv("TRAYHIP_WF_SLICES")) { slice_shift = 0u; while ((2u << slice_shift) <= (uint32_t)std::max(1, atoi(sl)) && (2u << slice_shift) <= 16u && (n_smp >> (slice_shift + 1u)) >= 1u) ++slice_shift; }
    const uint32_t n_items = tile_count << slice_shift;
    n_chunks = std::max(1u, std::min(n_chunks, n_items));
    const uint32_t n_slots = n_chunks * TR_BLOCK, n_active = n_slots;
    std::vector<float> pool_data((size_t)F_COUNT * n_slots, 0.0f);
    WfPool pool{pool_data.data(), n_slots, wf_seg_cap(n_chunks)};
    std::vector<uint32_t> moving_ids(std::max(n_moving, 1u), 0u);
    std::vector<float> xf_cache;
    if (moving && n_moving) {   // per-path transform cache, one column per pool slot (tray_scene_create)
        for (uint32_t i = 0; i < f->n_instances; ++i)
            if (f->instances[i].animated && f->instances[i].moving_slot < n_moving) moving_ids[f->instances[i].moving_slot] = i;
        xf_cache.assign((size_t)n_moving * TR_XF_REC * n_slots, 0.0f);
        e.d.xf_cache = xf_cache.data(); e.d.moving_ids = moving_ids.data(); e.d.n_moving = n_moving; e.d.xf_stride = n_moving; e.d.xf_cache_lanes = n_slots; e.d.xf_aos = 1u;
    }
    SparseXfTable table;   // TRAYHIP_EMU_XF_TABLE=1: the stage kernels index the frame's table by the path's time index (device_api.hip: xf_table_prepare's wavefront branch)
    if (moving && getenv("TRAYHIP_EMU_XF_TABLE") && atoi(getenv("TRAYHIP_EMU_XF_TABLE")) != 0) {
        if (!table.build(f, e.d.frame, moving_ids.data(), n_moving, tiles_xy, tile_count, spp, seed)) return -5;
        if (table.data) {
            e.d.moving_ids = moving_ids.data(); e.d.n_moving = n_moving; e.d.xf_tab = table.data; e.d.xf_tab_stride = table.stride;
            e.d.xf_cache = table.data; e.d.xf_table = 1u; e.d.xf_aos = 1u; e.d.xf_stride = table.stride;
        }
    }
    std::vector<WfChunk> chunks(n_chunks, WfChunk{WF_TILE_NEED, 0u});
    std::vector<float> bins((size_t)n_chunks * ROWBIN_SIZE, 0.0f);
    const size_t q_cap = (size_t)WF_SEGS * pool.seg_cap;
    const uint32_t q_blocks = (n_chunks + WF_SEGS - 1u) / WF_SEGS * WF_SEGS;   // grid of the one-thread-per-entry kernels (launch_wavefront)
    std::vector<uint32_t> queues((3 * WF_RAY_WORDS + 1) * q_cap + WF_QCTL_WORDS, 0u);   // ray queues A, B, C (the rays themselves), regeneration queue (slot indices)
    uint32_t* const qa = queues.data(), * const qb = qa + WF_RAY_WORDS * q_cap, * const qc = qb + WF_RAY_WORDS * q_cap, * const qr = qc + WF_RAY_WORDS * q_cap, * const qctl = qr + q_cap;
    uint32_t counters[2] = {0u, 0u};
    std::vector<DevStats> stats(WF_STAT_SLOTS);
    std::memset(stats.data(), 0, stats.size() * sizeof(DevStats));
    std::vector<uint2> tiles(tile_count);
    for (uint32_t i = 0; i < tile_count; ++i) tiles[i] = make_uint2(tiles_xy[2 * i], tiles_xy[2 * i + 1]);
    const uint32_t kf = key_frame_host(seed, e.d.frame);
    const uint32_t full = e.quad_words;
    if (lds_depth == 0 || lds_depth > full) lds_depth = full;
    trace_blocks = std::max(1u, std::min(trace_blocks, n_chunks));
    std::vector<uint32_t> overflow((size_t)(full + 64u) * trace_blocks * TR_BLOCK, 0u);
    const size_t fb_lds = (size_t)e.depth * TR_BLOCK * 4;
    const size_t dyn_lds = (size_t)lds_depth * TR_BLOCK * 4;
    const int feat = feature_set(e);
    // the material sort of the shading stage (default of the library for the compacted schedule; trace == 2 is the slot form without queues)
    if (trace != 0) return -6;
    const bool sorted = !(feat & FEAT_TEX);
    std::vector<uint32_t> kind_queues((size_t)WF_MAT_KINDS * q_cap, 0u);
    uint32_t kinds_present = 0;
    for (const DevMaterial& dm : e.mats) kinds_present |= 1u << dm.mat_kind;
    const uint64_t max_rounds = (uint64_t)((n_items + n_chunks - 1) / n_chunks) * (((uint64_t)n_smp + 3) / 4 * ((WF_FOLD_C ? 2u : 1u) * e.d.max_depth + 3) + 4) + 32;
    int rc = 0;
    uint64_t rounds = 0;
    // ray binning before the traversal stages, as launch_wavefront sets it up (TRAYHIP_WF_BIN: bit 0 = stage A, bit 1 = stage B)
    bool fused = sorted && WF_FOLD_C && WF_FUSED_DEFAULT != 0;   // launch_wavefront's choice of the shading form (TRAYHIP_WF_FUSED)
    if (const char* fe = getenv("TRAYHIP_WF_FUSED")) fused = sorted && WF_FOLD_C && atoi(fe) != 0;
    uint32_t bin_stages = WF_BIN_DEFAULT;
    if (const char* be = getenv("TRAYHIP_WF_BIN")) bin_stages = (uint32_t)std::max(0, atoi(be)) & 3u;
    std::vector<uint32_t> bin_ctl((size_t)2u * 2u * WF_SEGS * WF_BINS, 0u);
    const WfBinGrid bin_grid = f->n_top_nodes ? wf_bin_grid(f->top_nodes[0].bmin, f->top_nodes[0].bmax) : WfBinGrid{};
    const uint32_t bin_blocks = (pool.seg_cap + WF_BIN_EPB - 1u) / WF_BIN_EPB * WF_SEGS;
#define EMU_K(...) do { if (rc == 0) rc = launch_simt(__VA_ARGS__); } while (0)
#define EMU_ROUND(A, F)                                                                                                                     \
    do {                                                                                                                                    \
        EMU_K(n_chunks, TR_BLOCK, [&] { k_wf_advance<A>(e.d, pool, chunks.data(), bins.data(), tiles.data(), n_items, tile_count, 1u, spp, kf, rgbw, \
                                                         counters, counters + 1, stats.data(), qa, qr, qctl, slice_shift, smp_begin, smp_end); });                          \
        EMU_K(q_blocks, TR_BLOCK, [&] { k_wf_regen<A>(e.d, pool, chunks.data(), tiles.data(), tile_count, 1u, spp, kf, stats.data(), qr, qa, qctl, slice_shift); }); \
        if (WF_FOLD_C && (bin_stages & 1u)) { EMU_BIN(0, qa, qc, bin_ctl.data()); EMU_TRACE_STAGE(0, A, qc, qb); }   /* wf_round: the binned copy lies in the idle queue's buffer */ \
        else EMU_TRACE_STAGE(0, A, qa, qb);                                                                                                   \
        std::memset(qctl, 0, WF_QCTL_WORDS * sizeof(uint32_t));   /* wf_round: the control words are cleared between trace A and k_wf_begin */ \
        if (fused) {   /* wf_round: k_wf_sort + k_wf_shade_kind, then the occlusion stage */                                                  \
            EMU_K(n_chunks, TR_BLOCK, [&] { k_wf_sort<0>(e.d, pool, n_active, qctl, kind_queues.data()); });                                 \
            EMU_SHADE_KIND(A, TRAY_MAT_MATTE); EMU_SHADE_KIND(A, TRAY_MAT_PLASTIC); EMU_SHADE_KIND(A, TRAY_MAT_METAL); EMU_SHADE_KIND(A, TRAY_MAT_GLASS); \
            EMU_SHADE_KIND(A, TRAY_MAT_ROUGH_GLASS); EMU_SHADE_KIND(A, TRAY_MAT_SPECULAR_METAL); EMU_SHADE_KIND(A, TRAY_MAT_MERL);          \
            EMU_TRACE_STAGE(1, A, qb, qc);                                                                                                  \
            break;                                                                                                                          \
        }                                                                                                                                   \
        EMU_K(n_chunks, TR_BLOCK, [&] { k_wf_begin<A>(e.d, pool, n_active, stats.data(), qb, qctl, sorted ? kind_queues.data() : nullptr); }); \
        if (WF_FOLD_C && (bin_stages & 2u)) { EMU_BIN(1, qb, qa, bin_ctl.data() + 2u * WF_SEGS * WF_BINS); EMU_TRACE_STAGE(1, A, qa, qc); }     \
        else EMU_TRACE_STAGE(1, A, qb, qc);                                                                                                   \
        if (sorted) {   /* wf_round of kernels.hip: one kind-pure shading launch per material kind of the scene */                        \
            EMU_QUERY_KIND(A, TRAY_MAT_MATTE); EMU_QUERY_KIND(A, TRAY_MAT_PLASTIC); EMU_QUERY_KIND(A, TRAY_MAT_METAL); EMU_QUERY_KIND(A, TRAY_MAT_GLASS); \
            EMU_QUERY_KIND(A, TRAY_MAT_ROUGH_GLASS); EMU_QUERY_KIND(A, TRAY_MAT_SPECULAR_METAL); EMU_QUERY_KIND(A, TRAY_MAT_MERL);          \
        } else EMU_K(n_chunks, TR_BLOCK, [&] { k_wf_query<A, FEAT_ALL | FEAT_TEX>(e.d, pool, n_active, WF_FOLD_C ? nullptr : qc, qctl, stats.data(), qa); });  \
        if (!WF_FOLD_C) EMU_TRACE_STAGE(2, A, qc, qb);                                                                                                        \
    } while (0)
#define EMU_SHADE_KIND(A, K) do { if (kinds_present & (1u << K)) EMU_K(q_blocks, TR_BLOCK, [&] { k_wf_shade_kind<A, K>(e.d, pool, kind_queues.data(), qctl, stats.data(), qa, qb); }); } while (0)
#define EMU_QUERY_KIND(A, K) do { if (kinds_present & (1u << K)) EMU_K(q_blocks, TR_BLOCK, [&] { k_wf_query_kind<A, K>(e.d, pool, kind_queues.data(), WF_FOLD_C ? nullptr : qc, qctl, stats.data(), qa); }); } while (0)
#define EMU_TRACE_STAGE(S, A, Q, FB) /* FB: the queue buffer that is idle during stage S takes the deferred rays' records (wf_round) */                                                                                                          \
    do {                                                                                                                                    \
        const uint32_t fu_ = (S == 1 && fused) ? 1u : 0u;                                                                                   \
        EMU_K(trace_blocks, TR_BLOCK, [&] { k_wf_trace_dyn<S, A>(e.d, pool, Q, qctl, stats.data(), lds_depth, overflow.data(), FB, fu_); }, dyn_lds); \
        EMU_K(1u, TR_BLOCK, [&] { k_wf_trace_fallback<S, A>(e.d, pool, qctl, FB, fu_); }, fb_lds);                                    \
        g_wf_deferred += qctl[WF_FB_WORD + S];                                                                                              \
    } while (0)
#define EMU_BIN(S, Q, OUT, CTL) /* ray binning before stage S (wavefront.h: k_wf_bin_hist / k_wf_bin_scatter) */                          \
    do {                                                                                                                                    \
        EMU_K(bin_blocks, TR_BLOCK, [&] { k_wf_bin_hist<S>(pool, Q, qctl, CTL, bin_grid); });                                               \
        EMU_K(bin_blocks, TR_BLOCK, [&] { k_wf_bin_scatter<S>(pool, Q, OUT, qctl, CTL, bin_grid); });                                       \
    } while (0)
#define EMU_ROUND_F(A)                                                                                                                      \
    do {                                                                                                                                    \
        if (feat == FEAT_NONE) EMU_ROUND(A, FEAT_NONE); else if (feat == FEAT_MERL) EMU_ROUND(A, FEAT_MERL);                                \
        else if (feat == FEAT_SPEC) EMU_ROUND(A, FEAT_SPEC); else if (feat == (FEAT_MERL | FEAT_SPEC)) EMU_ROUND(A, FEAT_MERL | FEAT_SPEC);  \
        else if (feat == (FEAT_ALL | FEAT_TEX)) EMU_ROUND(A, FEAT_ALL | FEAT_TEX); else EMU_ROUND(A, FEAT_ALL);                                                                                                        \
    } while (0)
    std::memset(qctl, 0, WF_QCTL_WORDS * sizeof(uint32_t));
    while (rc == 0 && counters[1] < n_items) {
        std::fill(bin_ctl.begin(), bin_ctl.end(), 0u);
        if (moving) EMU_ROUND_F(1); else EMU_ROUND_F(0);
        if (++rounds > max_rounds) rc = -5;   // "wavefront schedule did not terminate"
    }
#undef EMU_ROUND_F
#undef EMU_BIN
#undef EMU_TRACE_STAGE
#undef EMU_QUERY_KIND
#undef EMU_SHADE_KIND
#undef EMU_ROUND
#undef EMU_K
    if (stats_out) {
        DevStats st{};
        for (const DevStats& a : stats) { st.samples += a.samples; st.vertices += a.vertices; st.rays += a.rays; }
        stats_out[0] = st.samples; stats_out[1] = st.vertices; stats_out[2] = st.rays; stats_out[3] = rounds;
    }
    return rc;
}

// emu_render_sampler under LowDiscrepancy over a sample range (scenes with an AnimatedMesh)
int emu_render_sampler_range(const TrayFlatScene* f, const uint32_t* tiles_xy, uint32_t tile_count, uint32_t spp, uint32_t smp_begin, uint32_t smp_end,
                             uint64_t seed, float* rgbw, uint32_t batch_tiles, unsigned long long* stats_out) {
    const uint32_t kind = TRAY_SAMPLER_LOW_DISCREPANCY, min_spp = spp, max_spp = spp;
    if (smp_begin == 0u && smp_end == spp) smp_end = 0u;
    EmuScene e;
    make_scene(f, e);
    const uint32_t kf = key_frame_host(seed, e.d.frame);
    bool moving = f->camera.animated != 0;
    for (uint32_t t_ = 0; t_ < f->n_textures; ++t_) moving = moving || f->textures[t_].n_frames >= 2u;
    for (uint32_t i = 0; i < f->n_instances; ++i) moving = moving || f->instances[i].animated != 0 || f->instances[i].emis_count >= 2;
    std::vector<uint2> tiles(tile_count);
    for (uint32_t i = 0; i < tile_count; ++i) tiles[i] = make_uint2(tiles_xy[2 * i], tiles_xy[2 * i + 1]);
    DevStats stats;
    std::memset(&stats, 0, sizeof stats);
    auto round_up = [](uint32_t v) { uint32_t p = 1; while (p < v && p < 0x80000000u) p <<= 1; return p; };
    SamplerPass sp{};
    sp.kind = kind; sp.min_spp = round_up(min_spp); sp.max_spp = round_up(max_spp);
    uint32_t rounds = 1;
    if (kind == TRAY_SAMPLER_ADAPTIVE) {
        if (sp.max_spp < sp.min_spp) return -1;
        sp.step = round_up((sp.max_spp - sp.min_spp) / 5u);
        while (sp.min_spp + (rounds - 1u) * sp.step < sp.max_spp) ++rounds;
        sp.lum_cap = sp.min_spp + (rounds - 1u) * sp.step;
    } else if (kind == TRAY_SAMPLER_UNIFORM) { sp.min_spp = sp.max_spp = 1u; sp.step = 1u; sp.lum_cap = 0u; }
    else if (kind == TRAY_SAMPLER_LOW_DISCREPANCY) { sp.max_spp = sp.min_spp; sp.step = 1u; sp.lum_cap = 0u; }   // (scenes with an AnimatedMesh: min_spp = the render's spp)
    else return -1;
    const uint32_t batch = batch_tiles ? std::min(batch_tiles, std::max(tile_count, 1u)) : std::max(tile_count, 1u);
    std::vector<uint32_t> px_state((size_t)batch * 64u);
    std::vector<float> px_avg((size_t)batch * 64u), px_lum((size_t)batch * 64u * std::max(sp.lum_cap, 1u));
    const uint32_t chunk = tile_count ? tile_count : 1u;
    int rc = 0;   // (the window is shared by the block's threads: a SIMT emulation, as for k_path_tiles)
    for (uint32_t item0 = 0; item0 < tile_count; item0 += batch) {
        const uint32_t n_items = std::min(batch, tile_count - item0), n_px = n_items * 64u;
        std::fill(px_state.begin(), px_state.end(), 0u); std::fill(px_avg.begin(), px_avg.end(), 0.0f);
        for (uint32_t j = 0; j < rounds; ++j) {
            sp.pass = j;
            sp.count = kind == TRAY_SAMPLER_ADAPTIVE ? (j == 0u ? sp.min_spp : sp.step) : sp.min_spp;
            sp.taken = kind == TRAY_SAMPLER_ADAPTIVE ? sp.min_spp + j * sp.step : 0u;
            sp.before = j == 0u ? 0u : sp.min_spp + (j - 1u) * sp.step;
            if (smp_end) sp.count = smp_end - smp_begin;   // (launch_sampler: a range of the LowDiscrepancy frame, from smp_begin on)
            const uint32_t per_tile = 64u * sp.count;   // launch_sampler's groups of tiles
            uint32_t group = std::max(1u, std::min<uint32_t>(SP_GROUP_MAX, 4096u / per_tile));
            if (const char* ge = getenv("TRAYHIP_SAMPLER_GROUP")) group = (uint32_t)std::max(1, std::min(SP_GROUP_MAX, atoi(ge)));   // (tests: ragged groups)
            const uint32_t grid = (n_items + group - 1u) / group;
#define EMU_SAMPLER_PASS(A, F) rc = launch_simt(grid, TR_BLOCK, [&] { k_sampler_pass<A, F>(e.d, tiles.data(), item0, n_items, chunk, 1u, kf, sp, px_state.data(), px_lum.data(), rgbw, &stats, group, smp_begin); })
            const bool lean = feature_set(e) == FEAT_NONE && f->integrator != TRAY_INTEGRATOR_WHITTED;   // launch_sampler's choice of the instantiation
            if (deforming(f)) { if (lean) EMU_SAMPLER_PASS(3, FEAT_NONE); else EMU_SAMPLER_PASS(3, FEAT_ALL | FEAT_TEX); }
            else if (moving) { if (lean) EMU_SAMPLER_PASS(2, FEAT_NONE); else EMU_SAMPLER_PASS(2, FEAT_ALL | FEAT_TEX); }
            else { if (lean) EMU_SAMPLER_PASS(0, FEAT_NONE); else EMU_SAMPLER_PASS(0, FEAT_ALL | FEAT_TEX); }
#undef EMU_SAMPLER_PASS
            if (rc != 0) return -3;
            if (kind == TRAY_SAMPLER_ADAPTIVE)
                launch((n_px + TR_BLOCK - 1) / TR_BLOCK, TR_BLOCK, [&] { k_sampler_decide(n_px, sp, px_state.data(), px_avg.data(), px_lum.data()); });
        }
    }
    if (stats_out) { stats_out[0] = stats.samples; stats_out[1] = stats.vertices; stats_out[2] = stats.rays; }
    return 0;
}

}  // extern "C"
