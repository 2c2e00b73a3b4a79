// What tray_scene_create decides about a scene before it launches anything: which scenes it refuses, which kernel instantiations the scene runs (ANIM,
// lobe feature set, light filter, material kinds), the schedule, the film, the traversal stack depth and the dynamic-LDS layout, the moving set. Host-only
// functions of a TrayFlatScene and its lowered materials -- no HIP call, no device scene, no environment: device_api.hip applies them (and its TRAYHIP_*
// overrides, between the steps) to a TrayDeviceScene, the host emulation (tests/emu) compiles this header under g++ and applies the same functions to its
// own launches. A per-scene decision is written here once. Include after kernels.hip (DevMaterial, FEAT_*, TR_BLOCK, TR_COOP_*, WIN_PLANE, TR_FLAT_MAX).
#pragma once

#include <string>
#include <utility>
#include <vector>

namespace tr_plan {

struct Refusal { int rc; std::string msg; };   // rc == TRAY_OK: the scene is one the device renders

// The refusals that need nothing but the scene. walk_mesh_trees: false for a frame update, which never reads the new scene's BVH<Triangle> nodes if it
// keeps the device's trees (scene_build validates them if it does not).
inline Refusal refuse(const TrayFlatScene* f, bool walk_mesh_trees) {
    if (f->abi_version != TRAY_ABI_VERSION) return {TRAY_E_INVALID, "tray_scene_create: ABI version mismatch"};
    if (f->n_lights == 0) return {TRAY_E_INVALID, "At least one light is required"};   // multithreaded.rs:39
    if (const std::string bad = tray::validate_flat_scene(f, walk_mesh_trees); !bad.empty()) return {TRAY_E_INVALID, "tray_scene_create: inconsistent scene: " + bad};
    if (f->film.width % 8 != 0 || f->film.height % 8 != 0 || f->film.width == 0 || f->film.height == 0)
        return {TRAY_E_INVALID, "Image dimensions not evenly divided by blocks of (8, 8)"};
    // the film windows (WIN_MAX, ROW_W, SP_WIN_MAX) hold a tile's write range with a 4-pixel halo: filter widths below 2.5. Every device
    // film writes within the write range of the sample's tile (kernels.hip: film_admit), so any width with floor(2 w) <= 4 fits.
    if (f->film.filter_pixel_w > 4 || f->film.filter_pixel_h > 4 || f->film.filter_pixel_w < 0 || f->film.filter_pixel_h < 0)
        return {TRAY_E_UNSUPPORTED, "reconstruction filters of width or height 2.5 and more are not supported by the LDS film window"};
    if (f->integrator > TRAY_INTEGRATOR_WHITTED) return {TRAY_E_INVALID, "unknown integrator"};
    if (f->integrator == TRAY_INTEGRATOR_WHITTED && f->max_depth > WH_MAX_DEPTH) return {TRAY_E_UNSUPPORTED, "whitted recursion depth > 16 is not supported"};
    if (f->integrator != TRAY_INTEGRATOR_WHITTED && f->max_depth > 15) return {TRAY_E_UNSUPPORTED, "pathtracer max_depth > 15 is not supported"};
    auto stack_ok = [&](uint32_t first, uint32_t count, bool moving) {   // spline stacks the device evaluates per ray
        if ((uint64_t)first + count > f->n_xf_levels) return false;
        for (uint32_t l = 0; moving && l < count; ++l) {
            const TrayXformLevel& lv = f->xf_levels[first + l];
            if (lv.kf_count < 2) continue;
            if (lv.degree > 3 || lv.knot_count != lv.kf_count + lv.degree + 1 || (uint64_t)lv.kf_first + lv.kf_count > f->n_keyframes ||
                (uint64_t)lv.knot_first + lv.knot_count > f->n_knots) return false;
        }
        return true;
    };
    if (!stack_ok(f->camera.xf_first, f->camera.xf_count, f->camera.animated != 0))
        return {TRAY_E_UNSUPPORTED, "camera keyframes: the device evaluates B-splines of degree <= 3 with consistent knot vectors"};
    for (uint32_t i = 0; i < f->n_instances; ++i) {
        const TrayInstance& in = f->instances[i];
        if (!stack_ok(in.xf_first, in.xf_count, in.animated != 0))
            return {TRAY_E_UNSUPPORTED, "instance keyframes: the device evaluates B-splines of degree <= 3 with consistent knot vectors"};
        if (in.emis_count && (uint64_t)in.emis_first + in.emis_count > f->n_color_keys) return {TRAY_E_INVALID, "instance references missing colour keys"};
        if (in.kind != TRAY_INST_POINT_EMITTER && in.material_id >= f->n_materials) return {TRAY_E_INVALID, "instance references a missing material"};
        if ((in.geom_type == TRAY_GEOM_MESH || in.geom_type == TRAY_GEOM_ANIMATED_MESH) && in.mesh_id >= f->n_meshes) return {TRAY_E_INVALID, "instance references a missing mesh"};
    }
    for (uint32_t i = 0; i < f->n_materials; ++i)
        if (f->materials[i].kind == TRAY_MAT_MERL && f->materials[i].table >= f->n_merl) return {TRAY_E_INVALID, "material references a missing MERL table"};
    return {TRAY_OK, ""};
}

// ANIM of the debug, sampler and first-hit kernels (2: the spline stacks evaluated at every use -- their grids are sized by the item count, not by a
// transform cache; 3: a scene with an AnimatedMesh)
inline int anim_debug(bool deforming, bool animated) { return deforming ? 3 : animated ? 2 : 0; }

struct ScenePlan {
    bool deforming = false;   // the scene holds an AnimatedMesh: every render runs k_sampler_pass<3> (dev_geom.h: ANIM = 3)
    bool animated = false;    // something needs ray.time: the <ANIM = 1> tile and stage kernels run
    int anim_debug() const { return tr_plan::anim_debug(deforming, animated); }
    uint32_t n_moving = 0;                // instances that move within the frame, and their ids by moving_slot (the per-path transform cache: dev_geom.h)
    std::vector<uint32_t> moving_ids;
    uint32_t xf_movable = 0;              // instances (+ camera) with a transform level of several keyframes: what ANY frame of the sequence can move
    int feat = FEAT_ALL;                  // lobe kinds of the materials that need the large kernels (dev_bsdf.h)
    uint32_t mat_kinds_present = 0;       // bit per TRAY_MAT_* kind among the materials
    bool light_filter = false;            // a sphere light or specular lobes: the tile kernel with mis_ray_filter (dev_integrator.h)
    bool film_rows_ok = false;            // the filter allows the row-binned film
    bool wavefront = false;               // the stage-kernel schedule (wavefront.h) instead of the tile megakernel
    uint32_t mesh_depth = 0, depth = 0;   // deepest BVH<Triangle>; traversal stack entries per lane
    uint32_t coop_offset = 0, win_offset = 0, stack_bytes = 0;   // dynamic LDS of every kernel that traverses: words in front of the cooperative area / the film window; bytes
};

inline void plan_motion(const TrayFlatScene* f, ScenePlan& p) {
    p.animated = f->camera.animated != 0;
    for (uint32_t t = 0; t < f->n_textures; ++t) p.animated = p.animated || f->textures[t].n_frames >= 2u;   // animated_image: sampled at ray.time
    for (uint32_t i = 0; i < f->n_instances; ++i) {
        const TrayInstance& in = f->instances[i];
        p.deforming = p.deforming || in.geom_type == TRAY_GEOM_ANIMATED_MESH;
        p.animated = p.animated || in.animated != 0 || in.emis_count >= 2 || in.geom_type == TRAY_GEOM_ANIMATED_MESH;
        if (in.animated) ++p.n_moving;
    }
    p.moving_ids.assign(p.n_moving, 0u);
    for (uint32_t i = 0; i < f->n_instances; ++i)
        if (f->instances[i].animated && f->instances[i].moving_slot < p.n_moving) p.moving_ids[f->instances[i].moving_slot] = i;
    // how many records per time index a later frame of this scene can need (launch_buffers_plan.h: table_ensure sizes the table's buffer once)
    auto movable = [&](uint32_t first, uint32_t count) {
        for (uint32_t l = first; l < first + count && l < f->n_xf_levels; ++l) if (f->xf_levels[l].kf_count > 1u) return true;
        return false;
    };
    p.xf_movable = movable(f->camera.xf_first, f->camera.xf_count) ? 1u : 0u;
    for (uint32_t i = 0; i < f->n_instances; ++i) if (movable(f->instances[i].xf_first, f->instances[i].xf_count)) p.xf_movable++;
}

// smallest kernel feature set that covers the materials, and their kinds
inline void plan_materials(const std::vector<DevMaterial>& mats, ScenePlan& p) {
    int feat = FEAT_NONE;
    for (const DevMaterial& dm : mats) {
        for (uint32_t l = 0; l < dm.n_lobes && l < 2u; ++l) {
            const uint32_t k = dm.lobe[l].kind;
            if (k == LB_MERL) feat |= FEAT_MERL;
            if (k == LB_MF_TRANS) feat |= FEAT_MF_TRANS;
            if (k == LB_SPEC_REFL_DIEL || k == LB_SPEC_REFL_COND || k == LB_SPEC_TRANS || k == LB_TS_COND) feat |= FEAT_SPEC;
        }
        p.mat_kinds_present |= 1u << dm.mat_kind;
    }
    p.feat = (feat & FEAT_MF_TRANS) ? FEAT_ALL : feat;
    for (const DevMaterial& dm : mats)   // lobes of textured materials are only known per hit; GGX lives in the same instantiation
        if (dm.textured || dm.microfacet == TRAY_MF_GGX) p.feat = FEAT_ALL | FEAT_TEX;
}
inline void plan_light_filter(const TrayFlatScene* f, ScenePlan& p) {   // (after p.feat)
    p.light_filter = (p.feat & FEAT_SPEC) != 0;
    for (uint32_t l = 0; l < f->n_lights; ++l)
        if (f->instances[f->lights[l]].kind != TRAY_INST_POINT_EMITTER && f->instances[f->lights[l]].geom_type == TRAY_GEOM_SPHERE) p.light_filter = true;
}

// row-binned film needs: separable table, filter_h == 2 (class = eighth of a pixel), consistent factors
inline bool film_rows_ok(const TrayFilm& film) {
    bool ok = film.separable != 0 && film.filter_h == 2.0f && film.inv_h == 0.5f && film.filter_pixel_h == 4;
    for (int y = 0; ok && y < TRAY_FILTER_TABLE_SIZE; ++y)
        for (int x = 0; x < TRAY_FILTER_TABLE_SIZE; ++x)
            if (film.table[y * TRAY_FILTER_TABLE_SIZE + x] != film.table_x[x] * film.table_y[y]) { ok = false; break; }
    return ok;
}

// Schedule: the tile megakernel for scenes its flat instance loop covers, the wavefront stage kernels (compacted ray queues, persistent traversal with
// dynamic fetch) for scenes that go through BVH<Instance>. wavefront_can: the Whitted recursion runs inside the tile kernel only (dev_whitted.h), and
// k_sampler_pass<3> renders the scenes with an AnimatedMesh (launch_tiles). trees_ok: a tree the quad-record traversal cannot take (a box with min > max
// or NaN -- BBox::new() is +inf / -inf in the reference --, a mesh beyond the 23-bit descriptors: host/gates.hpp) renders through the tile kernel's binary
// traversal, which is the reference's, instead of failing at render time.
inline bool wavefront_can(const TrayFlatScene* f, const ScenePlan& p) { return f->integrator != TRAY_INTEGRATOR_WHITTED && !p.deforming; }
inline bool wavefront(const TrayFlatScene* f, bool trees_ok, const ScenePlan& p) { return f->n_instances > TR_FLAT_MAX && trees_ok && wavefront_can(f, p); }

// leaf(node, depth) for every leaf of a binary BVH in the reference's layout (left child next, right child at `offset`); the root's depth is 1
template <class F>
inline void for_each_leaf(const TrayBvhNode* nodes, uint32_t n, F&& leaf) {
    std::vector<std::pair<uint32_t, uint32_t>> st;   // node, depth
    if (n) st.push_back({0u, 1u});
    while (!st.empty()) {
        auto [idx, dep] = st.back();
        st.pop_back();
        if (idx >= n) continue;
        if (nodes[idx].count == 0) { st.push_back({idx + 1, dep + 1}); st.push_back({nodes[idx].offset, dep + 1}); }
        else leaf(nodes[idx], dep);
    }
}
inline uint32_t bvh_depth(const TrayBvhNode* nodes, uint32_t n) {
    uint32_t best = 0;
    for_each_leaf(nodes, n, [&](const TrayBvhNode&, uint32_t dep) { best = std::max(best, dep); });
    return best;
}
// deepest node of every BVH<Triangle> (a frame update that keeps the device's trees keeps these: the walk over the 6.2 M nodes of the tr15 stand-in's
// meshes was 80 ms per frame)
inline std::vector<uint32_t> mesh_depths(const TrayFlatScene* f) {
    std::vector<uint32_t> d(f->n_meshes, 0u);
    for (uint32_t m = 0; m < f->n_meshes; ++m) d[m] = bvh_depth(f->mesh_nodes + f->meshes[m].node_offset, f->meshes[m].node_count);
    return d;
}

// Traversal stack entries per lane. The per-lane BVH<Triangle> traversal keeps one pending far child per level. The two-level traversal (scenes the flat
// instance loop serves need it too: rays with tied candidates are re-traced through BVH<Instance>) takes the exact worst case over the instances: while
// instance j of a BVH<Instance> leaf at depth d is traversed the stack holds the pending far children of the top-level path (d - 1), the leaf's later
// instances, the exit-mesh sentinel and the pending far children inside the mesh (its depth - 1). One spare entry; at least 4.
inline void plan_stacks(const TrayFlatScene* f, const std::vector<uint32_t>& mesh_depths, ScenePlan& p) {
    p.mesh_depth = 0;
    for (uint32_t m = 0; m < f->n_meshes; ++m) p.mesh_depth = std::max(p.mesh_depth, mesh_depths[m]);
    uint32_t worst = 0;
    for_each_leaf(f->top_nodes, f->n_top_nodes, [&](const TrayBvhNode& nd, uint32_t dep) {
        for (uint32_t j = 0; j < nd.count; ++j) {
            uint32_t need = (dep - 1) + (nd.count - 1 - j);
            if (nd.offset + j < f->n_top_order) {
                const TrayInstance& in = f->instances[f->top_order[nd.offset + j]];
                if ((in.geom_type == TRAY_GEOM_MESH || in.geom_type == TRAY_GEOM_ANIMATED_MESH) && in.mesh_id < f->n_meshes) need += 1 + (mesh_depths[in.mesh_id] > 0 ? mesh_depths[in.mesh_id] - 1 : 0);
            }
            worst = std::max(worst, need);
        }
        worst = std::max(worst, dep - 1 + nd.count);   // right after the leaf queued its instances
    });
    p.depth = std::max(std::max(p.mesh_depth + 1, worst + 1), 4u);
}

// Dynamic-LDS layout (after wavefront and depth): the stacks; behind them, per wave, the cooperative test of small meshes in the flat instance loop
// (dev_geom.h: mesh_leaf_coop; moving scenes too); the tile kernel's film window over the stacks for the row-binned film, behind everything else
// otherwise (k_path_tiles).
inline void plan_lds(const TrayFlatScene* f, bool coop, bool film_rows, ScenePlan& p) {
    p.stack_bytes = p.depth * TR_BLOCK * (uint32_t)sizeof(uint32_t);
    bool single_leaf = false;
    for (uint32_t m = 0; m < f->n_meshes; ++m) single_leaf = single_leaf || f->meshes[m].tri_count <= TR_COOP_MAX_TRIS;
    p.coop_offset = 0u;
    if (coop && single_leaf && !p.wavefront && f->n_instances <= TR_FLAT_MAX) {
        p.coop_offset = p.depth * TR_BLOCK;
        p.stack_bytes += (TR_BLOCK / 64) * TR_COOP_WORDS * (uint32_t)sizeof(float);
    }
    const uint32_t win_bytes = 4u * WIN_PLANE * (uint32_t)sizeof(float);
    if (film_rows) { p.win_offset = 0u; p.stack_bytes = std::max(p.stack_bytes, win_bytes); }
    else { p.win_offset = p.stack_bytes / (uint32_t)sizeof(uint32_t); p.stack_bytes += win_bytes; }
}

}  // namespace tr_plan
