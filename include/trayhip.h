/*
 * trayhip.h — C ABI of libtrayhip.so, the MI355X (gfx950) path-tracing core that
 * replaces tray_rust's tile worker.
 *
 * Drop-in seam (reference, /root/reference):
 *   trait Exec::render(&mut self, &mut Scene, &mut RenderTarget, &Config)   src/exec/mod.rs:41-49
 *   MultiThreaded::render_parallel + thread_work                            src/exec/multithreaded.rs:30-114
 *   Scene::load_file                                                        src/scene.rs:101-145
 *   RenderTarget::{write,get_render,get_renderf32}                          src/film/render_target.rs:77,185,243
 *   film::Image::add_pixels (merge of per-worker RGBW)                      src/film/image.rs:21-34
 *   BlockQueue::new (Morton tile list + select_blocks)                      src/sampler/block_queue.rs:28-48
 *
 * Everything is plain C: PODs, pointers and sizes. No torch / C++ types cross this line.
 * All entry points return 0 on success and a negative TRAY_E_* code on failure; the message is
 * available from tray_last_error() (thread local). Nothing aborts across the ABI: the reference's
 * panics (scene.rs:104-136, block_queue.rs:29-31, multithreaded.rs:39) become checked errors.
 *
 * The same TrayFlatScene POD is what the CPU oracle (oracle/, test infrastructure only) consumes,
 * so oracle and HIP path are fed bit-identical scene data.
 */
#ifndef TRAYHIP_H
#define TRAYHIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRAY_ABI_VERSION 4

enum {
    TRAY_OK = 0,
    TRAY_E_INVALID = -1,   /* bad argument / precondition (reference would panic) */
    TRAY_E_IO = -2,        /* file could not be opened / read */
    TRAY_E_PARSE = -3,     /* JSON / OBJ / MERL parse error */
    TRAY_E_UNSUPPORTED = -4, /* feature outside the hot-path scope */
    TRAY_E_DEVICE = -5,    /* HIP runtime error */
    TRAY_E_NOMEM = -6
};

/* ---------------------------------------------------------------- flat scene (SoA/AoS PODs) */

/* Flattened BVH2 node, 32 B: reference FlatNode (src/geometry/bvh.rs:278-295).
 * count > 0  : leaf, prims ordered[offset .. offset+count)
 * count == 0 : interior, first child = this+1, second child = offset, split axis = axis */
typedef struct TrayBvhNode {
    float bmin[3];
    float bmax[3];
    uint32_t offset;
    uint16_t count;
    uint8_t axis;
    uint8_t pad;
} TrayBvhNode;

/* Hot triangle record (48 B, 3 x float4) in mesh-BVH leaf order: positions only.
 * Reference Triangle{a,b,c,positions} (src/geometry/mesh.rs:88-111), pre-gathered. */
typedef struct TrayTriVerts {
    float pa[3]; uint32_t tri_id;  /* index of this triangle in the OBJ order (for debugging) */
    float pb[3]; uint32_t pad0;
    float pc[3]; uint32_t pad1;
} TrayTriVerts;

/* Cold triangle record (64 B): shading normals + texcoords, read once for the final hit. */
typedef struct TrayTriAttrs {
    float na[3], nb[3], nc[3];
    float ta[2], tb[2], tc[2];
    float pad;
} TrayTriAttrs;

typedef struct TrayMesh {
    uint32_t node_offset;  /* into TrayFlatScene.mesh_nodes */
    uint32_t node_count;
    uint32_t tri_offset;   /* into tri_verts / tri_attrs (leaf order) */
    uint32_t tri_count;
} TrayMesh;

/* AnimatedMesh (src/geometry/animated_mesh.rs:93-143): a mesh whose vertex positions, normals and texcoords are interpolated linearly
 * between keyframes at ray.time (AnimatedMeshData::position / normal / texcoord, :72-107), behind ONE BVH<AnimatedTriangle> built over the
 * triangles' bounds at times[0] and times[1] (AnimatedMesh::new, :124-126 -- Boundable::update_deformation, :140-142, has no caller in the
 * reference, so that tree serves every frame: quirk Q13). meshes[m] describes the tree and ONE keyframe's triangles (tri_count); keyframe k
 * of the mesh lies at tri_verts / tri_attrs [tri_offset + k * tri_count ...], all in the leaf order of that tree; mesh_keys[m] names the
 * keyframe times. n_keys == 1 for a plain Mesh. */
typedef struct TrayMeshKeys {
    uint32_t n_keys;       /* >= 2 for an animated mesh */
    uint32_t time_first;   /* into TrayFlatScene.key_times (ascending per mesh) */
} TrayMeshKeys;

enum { TRAY_GEOM_SPHERE = 0, TRAY_GEOM_DISK = 1, TRAY_GEOM_RECT = 2, TRAY_GEOM_MESH = 3, TRAY_GEOM_NONE = 4, TRAY_GEOM_ANIMATED_MESH = 5 };
enum { TRAY_INST_RECEIVER = 0, TRAY_INST_AREA_EMITTER = 1, TRAY_INST_POINT_EMITTER = 2 };

/* One Instance (src/geometry/instance.rs:72-105) with its transform evaluated for the frame.
 * mat/inv are the full row-major 4x4 of Transform{mat,inv} (src/linalg/transform.rs:11-14) built
 * in the reference's order: per spline level translate*rot*scale (keyframe.rs:60-63), stacked
 * object-first (animated_transform.rs:40-56). Row 3 is kept because Transform*Point divides by w
 * only when |w-1| < eps (transform.rs:211-215). */
typedef struct TrayInstance {
    uint32_t kind;        /* TRAY_INST_* */
    uint32_t geom_type;   /* TRAY_GEOM_* */
    uint32_t mesh_id;     /* valid for TRAY_GEOM_MESH */
    uint32_t material_id; /* 0xffffffff for point emitters */
    float geom_params[4]; /* sphere: radius | disk: radius, inner_radius | rect: width, height */
    float emission[4];    /* AnimatedColor::color(shutter_open) (rgb, a); exact for every ray when emis_count <= 1 */
    float mat[16];        /* transform(shutter_open); exact for every ray when animated == 0 */
    float inv[16];
    uint32_t light_index; /* index in lights[] or 0xffffffff */
    uint32_t xf_first;    /* first TrayXformLevel of this instance's spline stack */
    uint32_t xf_count;    /* number of levels (object first, then group parents) */
    uint32_t animated;    /* 1 => some level varies while the shutter is open: evaluate the stack at ray.time
                           * (receiver.rs:30, emitter.rs:122,161,169,190) */
    uint32_t emis_first;  /* AnimatedColor keyframes in color_keys[] (film/animated_color.rs:45-49), sorted by time */
    uint32_t emis_count;
    uint32_t moving_slot; /* index among the animated instances of this frame (0xffffffff if not animated) */
    uint32_t pad;
} TrayInstance;

/* TRS keyframe (src/linalg/keyframe.rs:13-17) */
typedef struct TrayKeyframe {
    float translation[3];
    float rotation[4];    /* quaternion v.xyz, w */
    float scaling[3];
} TrayKeyframe;

/* One B-spline level of an AnimatedTransform (src/linalg/animated_transform.rs:15-19).
 * BSpline<Keyframe> of the bspline crate (0.2.2, not vendored by the reference): clamped de Boor evaluation over the
 * sorted knot vector, domain (knots[degree], knots[n_knots-1-degree]); a level with ONE control point is a constant
 * (animated_transform.rs:47-48) whose Transform is stored in mat/inv. */
typedef struct TrayXformLevel {
    uint32_t kf_first, kf_count;     /* control points in keyframes[] */
    uint32_t knot_first, knot_count; /* knots in knots[] (sorted ascending) */
    uint32_t degree;
    uint32_t is_const;               /* 1 => the level has the same value for every ray of this frame: one control point, or
                                      * the open shutter lies outside the knot domain, where transform() clamps the time
                                      * (animated_transform.rs:49-50). mat/inv hold that value. */
    uint32_t pad[2];
    float mat[16];                   /* Keyframe::transform() of the constant level (keyframe.rs:60-63) */
    float inv[16];
} TrayXformLevel;

/* ColorKeyframe (src/film/animated_color.rs:10-14) */
typedef struct TrayColorKey {
    float color[4];
    float time;
    float pad[3];
} TrayColorKey;

enum {
    TRAY_MAT_MATTE = 0, TRAY_MAT_PLASTIC = 1, TRAY_MAT_METAL = 2, TRAY_MAT_GLASS = 3,
    TRAY_MAT_ROUGH_GLASS = 4, TRAY_MAT_SPECULAR_METAL = 5, TRAY_MAT_MERL = 6
};

/* Image textures (src/texture/image.rs:9-47, animated_image.rs:7-58; loader scene.rs:317-394). A texture is one frame (type
 * "image") or >= 2 keyed frames ("animated_image", "movie": lerp between the two frames around ray.time, the first / last frame
 * outside the keys). Frames are RGBA8 as image::DynamicImage::get_pixel presents them (row 0 on top; grey -> l,l,l,255). */
typedef struct TrayTexture {
    uint32_t first_frame, n_frames;   /* in tex_frames[] */
} TrayTexture;
typedef struct TrayTexFrame {
    float time;                        /* keyframe time (0 for a plain image) */
    uint32_t width, height;
    uint32_t pad;
    uint64_t offset;                   /* byte offset of the frame's width*height*4 bytes in tex_data */
} TrayTexFrame;
#define TRAY_NO_TEXTURE 0xffffffffu

/* Closed lowering of the reference's Material trait objects (src/material/ *.rs). Every parameter is a Texture in the
 * reference (texture/mod.rs:15-20): here a constant (c0 / c1 / f0 / f1; scalars read from constant colours are their
 * luminance, texture/mod.rs:70-72) or, when the matching tex_* field is not TRAY_NO_TEXTURE, an image texture sampled at the
 * hit's (u, v, time) -- sample_color for colour parameters, sample_f32 (red channel) for scalar ones.
 *   MATTE          c0 = diffuse,            f0 = roughness            (matte.rs:52-65)
 *   PLASTIC        c0 = diffuse, c1 = gloss, f0 = roughness           (plastic.rs:59-88)
 *   METAL          c0 = eta, c1 = k,        f0 = roughness            (metal.rs:56-67)
 *   GLASS          c0 = reflect, c1 = transmit, f0 = eta              (glass.rs:51-78)
 *   ROUGH_GLASS    c0 = reflect, c1 = transmit, f0 = eta, f1 = roughness (rough_glass.rs:57-85)
 *   SPECULAR_METAL c0 = eta, c1 = k                                   (specular_metal.rs:49-58)
 *   MERL           table = index into merl tables                     (material/merl.rs:88-92) */
typedef struct TrayMaterial {
    uint32_t kind;
    uint32_t table;
    float f0, f1;
    float c0[4];
    float c1[4];
    uint32_t tex_c0, tex_c1, tex_f0, tex_f1;   /* texture ids or TRAY_NO_TEXTURE */
    uint32_t microfacet;   /* TRAY_MF_*: the MicrofacetDistribution of plastic / metal / rough_glass. The reference's materials
                            * always build Beckmann (plastic.rs:83, metal.rs:63, rough_glass.rs:73); its GGX (bxdf/microfacet/
                            * ggx.rs:20-57) is selected here by the scene-file extension key "microfacet": "ggx" */
    uint32_t pad[3];
} TrayMaterial;
enum { TRAY_MF_BECKMANN = 0, TRAY_MF_GGX = 1 };
/* Integrator (src/integrator): the Path tracer (path.rs) or NormalsDebug (normals_debug.rs:28-33: (bsdf.n + 1) / 2 of the
 * camera ray's hit), or Whitted (whitted.rs:41-68 with Integrator::specular_reflection / specular_transmission, mod.rs:49-97). */
enum { TRAY_INTEGRATOR_PATH = 0, TRAY_INTEGRATOR_NORMALS_DEBUG = 1,
       TRAY_INTEGRATOR_WHITTED = 2 };   /* integrator/whitted.rs: max_depth = the recursion limit (<= 16), min_depth unused */

/* MERL table header: 90*90*180 RGB-interleaved f32, already scaled (material/merl.rs:60-82) */
typedef struct TrayMerlTable {
    uint64_t offset;  /* float offset into merl_data */
    uint32_t n_theta_h, n_theta_d, n_phi_d;
    uint32_t pad;
} TrayMerlTable;

/* Camera for one frame (src/film/camera.rs:64-157).
 * raster_to_cam = (proj_div_inv * raster_screen).mat, a genuinely projective 4x4 (Q5). */
typedef struct TrayCamera {
    float raster_to_cam[16];
    float scaling[3];
    float shutter_open, shutter_close;
    float cam_world[16];   /* cam_world.transform(shutter_open).mat; exact for every ray when animated == 0 */
    uint32_t animated;     /* 1 => cam_world.transform(frame_time) is evaluated per ray (camera.rs:156) */
    uint32_t xf_first, xf_count;
} TrayCamera;

#define TRAY_FILTER_TABLE_SIZE 16

/* Film + reconstruction filter (src/film/render_target.rs:41-75) */
typedef struct TrayFilm {
    uint32_t width, height;
    float filter_w, filter_h, inv_w, inv_h;
    int32_t filter_pixel_w, filter_pixel_h;   /* floor(w/0.5), floor(h/0.5) */
    float table[TRAY_FILTER_TABLE_SIZE * TRAY_FILTER_TABLE_SIZE];
    /* 1-D factors when the filter is a product of per-axis weights (both reference filters are):
     * table[y*16 + x] == table_x[x] * table_y[y] in f32. separable = 0 if no such factors exist. */
    float table_x[TRAY_FILTER_TABLE_SIZE];
    float table_y[TRAY_FILTER_TABLE_SIZE];
    uint32_t separable;
} TrayFilm;

typedef struct TrayFlatScene {
    uint32_t abi_version;
    uint32_t frame;
    TrayFilm film;
    TrayCamera camera;
    uint32_t min_depth, max_depth;       /* Path integrator (src/integrator/path.rs:33-43) */

    uint32_t n_instances;   const TrayInstance* instances;
    uint32_t n_top_nodes;   const TrayBvhNode* top_nodes;       /* BVH<Instance>, leaf <= 4 */
    uint32_t n_top_order;   const uint32_t* top_order;          /* ordered_geom of the top BVH */
    uint32_t n_meshes;      const TrayMesh* meshes;
    uint32_t n_mesh_nodes;  const TrayBvhNode* mesh_nodes;      /* all BVH<Triangle>, leaf <= 16 */
    uint32_t n_tris;        const TrayTriVerts* tri_verts;      /* leaf order, per mesh */
                            const TrayTriAttrs* tri_attrs;
    uint32_t n_materials;   const TrayMaterial* materials;
    uint32_t n_merl;        const TrayMerlTable* merl_tables;
    uint64_t n_merl_floats; const float* merl_data;
    uint32_t n_lights;      const uint32_t* lights;             /* instance ids, scene order */
    uint32_t n_xf_levels;   const TrayXformLevel* xf_levels;
    uint32_t n_keyframes;   const TrayKeyframe* keyframes;
    uint32_t n_knots;       const float* knots;
    uint32_t n_color_keys;  const TrayColorKey* color_keys;
    uint32_t animated;      /* 1 if the camera, any instance transform or any emission varies over the open shutter */
    uint32_t integrator;    /* TRAY_INTEGRATOR_* */
    uint32_t n_textures;    const TrayTexture* textures;
    uint32_t n_tex_frames;  const TrayTexFrame* tex_frames;
    uint64_t n_tex_bytes;   const uint8_t* tex_data;            /* RGBA8 texels of all frames */
    uint32_t n_mesh_keys;   const TrayMeshKeys* mesh_keys;      /* n_meshes entries, or 0 / NULL when no mesh is animated */
    uint32_t n_key_times;   const float* key_times;
} TrayFlatScene;

/* ---------------------------------------------------------------- host side: loader (scene.rs) */

typedef struct TrayHostScene TrayHostScene;

typedef struct TraySceneInfo {
    uint32_t width, height;
    uint32_t spp;                /* film.samples as written in the file */
    uint32_t frames, start_frame, end_frame;
    float scene_time;
    uint32_t n_instances, n_lights, n_meshes, n_tris;
} TraySceneInfo;

/* Scene::load_file (src/scene.rs:101-145). The JSON schema is the reference's. */
int tray_scene_load_file(const char* path, TrayHostScene** out);
/* Same, from an in-memory JSON string; base_dir resolves relative mesh / MERL paths. */
int tray_scene_load_string(const char* json, const char* base_dir, TrayHostScene** out);
int tray_host_scene_info(const TrayHostScene* s, TraySceneInfo* info);
/* Scene::update_frame (scene.rs:152-176) + flattening for frame `frame`: camera shutter, top-level
 * BVH rebuilt over the shutter interval, per-instance matrices. The returned view borrows from `s`
 * and is valid until the next flatten / free on `s`. */
int tray_host_scene_flatten(TrayHostScene* s, uint32_t frame, const TrayFlatScene** out);
void tray_host_scene_free(TrayHostScene* s);

/* BlockQueue::new (src/sampler/block_queue.rs:28-48): 8x8 tiles sorted by Morton code of the
 * tile index. Writes up to `cap` (x,y) tile coordinates into xy (2*u32 each), returns the number
 * of tiles through n_out. select (start,count) applies after sorting; count 0 = all. */
int tray_block_queue(uint32_t width, uint32_t height, uint32_t select_start, uint32_t select_count,
                     uint32_t* xy, uint32_t cap, uint32_t* n_out);

/* LowDiscrepancy::new rounding (src/sampler/ld.rs:22-25) */
uint32_t tray_round_spp(uint32_t spp);

/* RenderTarget::get_render (render_target.rs:185-210): RGBW f32 -> sRGB8 (3 bytes / pixel). */
int tray_resolve_srgb8(const float* rgbw, uint32_t width, uint32_t height, uint8_t* rgb8);

/* ---------------------------------------------------------------- device side: the tile worker */

typedef struct TrayDeviceScene TrayDeviceScene;

/* Bind the calling thread's library state to HIP device `device` (one process per GPU). */
int tray_init(int device);
int tray_device_count(int* n);

/* Deep-copies the flat scene to the current device. */
int tray_scene_create(const TrayFlatScene* flat, TrayDeviceScene** out);
/* Scene::update_frame (src/scene.rs:152-176; the frame loop of src/main.rs:91-106 keeps the Scene and rebuilds the instance
 * transforms and BVH<Instance> per frame): `flat` is the SAME scene flattened at another frame. Instances, BVH<Instance>, camera,
 * spline tables, emission keys and the set of moving instances are uploaded anew; meshes, MERL tables, textures and the tile queue stay
 * on the device, and so do the launch buffers -- the wavefront pool / queues, the per-path transform cache and the transform table's buffer --
 * as far as the new frame can use them: the cache if it has room for the frame's moving instances on the same schedule, the table's buffer
 * (rebuilt by the frame's first launch that reads it, replaced if it is too small), the pool if the traversal stacks and the kernels are the
 * same and it is no larger than the per-path cache's lanes or the pool size wished for -- or was sized for launches that read the table.
 * Waits for the device to be idle. On an error the handle can only be passed to tray_scene_destroy. */
int tray_scene_update_frame(TrayDeviceScene* s, const TrayFlatScene* flat);
void tray_scene_destroy(TrayDeviceScene* s);

/* thread_work over tiles [tile_start, tile_start+tile_count) of the Morton queue
 * (exec/multithreaded.rs:72-114 with Config.select_blocks, exec/mod.rs:25-27).
 * Adds filtered samples into rgbw_dev: device pointer, width*height*4 f32, the layout of
 * RenderTarget::get_renderf32 (render_target.rs:243-266). Asynchronous on `stream`
 * (a hipStream_t; NULL = default stream). spp must already be a power of two (it is not used when tray_scene_set_sampler chose
 * Uniform or Adaptive). */
/* tile_count == 0 selects the whole queue whatever tile_start is (BlockQueue::new, block_queue.rs:39-41).
 * ONE render may be in flight per TrayDeviceScene: the tile counter, the statistics, the per-path transform cache, the wavefront
 * pool and queues and the timing events belong to the handle. Calls on one handle must be serialised by the caller (the
 * reference blocks inside Exec::render too, multithreaded.rs:54-70); use one handle per stream for concurrent renders.
 * Scenes that traverse BVH<Instance> (more than 16 instances) run the wavefront schedule: it polls for completion (the call
 * returns when the tiles are done), uses one internal stream beside `stream` (forked from and joined back to it with events) and
 * returns TRAY_E_UNSUPPORTED for a mesh of more than 8 388 607 BVH nodes or triangles (its traversal keeps a node as a 32-bit word).
 * Its path pool is sized for the device: up to 32 M paths in flight (8.9 GB + 5 GB of queues and film bins) and, for a scene with instances that
 * move while the shutter is open, 112 B per path and such instance of cached transforms within two fifths of the free memory (TRAYHIP_WF_SLOTS /
 * TRAYHIP_XF_CACHE_BYTES bound both; a failed allocation is TRAY_E_NOMEM). */
int tray_render_tiles_device(TrayDeviceScene* s, uint32_t tile_start, uint32_t tile_count,
                             uint32_t spp, uint64_t seed, float* rgbw_dev, void* stream);

/* Multi-GPU sharding of one frame: shard g of n_shards renders chunks g, g+n_shards, g+2*n_shards...
 * of the Morton queue, chunk_tiles tiles per chunk (round-robin instead of the reference's contiguous
 * per = n/workers split, src/exec/distrib/master.rs:91-93,218-227, for load balance; per-pixel results
 * do not depend on the partition because the RNG is keyed by pixel and sample). The per-shard buffers
 * are merged by addition (film/image.rs:21-50), e.g. ncclReduce(sum). */
int tray_render_shard_device(TrayDeviceScene* s, uint32_t shard, uint32_t n_shards, uint32_t chunk_tiles,
                             uint32_t spp, uint64_t seed, float* rgbw_dev, void* stream);

/* The samples [sample_begin, sample_end) of every pixel of tiles [tile_start, tile_start+tile_count) of a spp-sample
 * LowDiscrepancy frame, added into rgbw_dev. Ranges that partition [0, spp) add up to tray_render_tiles_device's film. */
/* Sample s of a pixel is the sample the whole frame traces at s (ld.rs:33-52 draws sample_02(i) / van_der_corput(i) of the frame's
 * spp-long sequences; TRAY-CBRNG keys the rest by (seed, frame, pixel, s)), so a range is a progressive pass or a GPU's share of the
 * samples, and the films of ranges are merged by addition (film/image.rs:21-50). tile_count == 0 selects the whole queue, as in
 * tray_render_tiles_device; [0, spp) is that call. TrayKernelTiming counts the range's samples only. Returns TRAY_E_INVALID unless
 * sample_begin < sample_end <= spp and spp is a power of two, TRAY_E_UNSUPPORTED while tray_scene_set_sampler has chosen Uniform or
 * Adaptive (an Adaptive pass depends on the samples taken before it). */
int tray_render_samples_device(TrayDeviceScene* s, uint32_t tile_start, uint32_t tile_count, uint32_t spp,
                               uint32_t sample_begin, uint32_t sample_end, uint64_t seed, float* rgbw_dev, void* stream);

/* First-hit feature films: where the camera rays of the samples [sample_begin, sample_end) of tray_render_samples_device's frame first land,
 * added into three RGBW films of their own (get_renderf32 layout, zeroed by the caller): albedo, shading normal, depth.
 * - Sample. Camera sample (px, py, s) of the spp-sample LowDiscrepancy frame under `seed` is (sx, sy, time), the result of pixel_sample; its
 *   ray is camera_ray(sx, sy, time), its hit Scene::intersect's (scene.rs:148-150): the position, ray and first hit that
 *   tray_render_samples_device traces for that sample.
 * - hit is 1 or 0.
 * - albedo: (0, 0, 0) on a miss. MATTE and PLASTIC: the material's c0 -- the constant, or Texture::sample_color of tex_c0 at the hit's
 *   (u, v, ray.time). Every other material kind, and an instance with material_id == 0xffffffff: (1, 1, 1). No clamping; an emitter's
 *   material counts like any other.
 * - normal: TrayHit.n as tray_debug_intersect reports it -- world space, not flipped towards the ray --, 0 on a miss.
 * - depth: (TrayHit.t, hit, 0), with t = 0 on a miss: the resolved film's r / g is the mean distance over the samples that hit, g the coverage.
 * - Films. Each of the three colours goes through RenderTarget::write at (sx, sy) (render_target.rs:77-165), as a radiance sample does, so the
 *   three w planes are the colour film's of the same samples up to the order of the f32 sums, and the films line up with the colour films
 *   weight for weight. Ranges that partition [0, spp) add up; both halves may go into one film.
 * tile_count == 0 selects the whole queue. One kernel launch on `stream`, asynchronous, no host synchronisation, whatever schedule renders the
 * scene; TrayKernelTiming is not touched. Returns TRAY_E_INVALID under tray_render_samples_device's rules, if a film is null, if two of the
 * three films are the same buffer or if a film is not 16-byte aligned; TRAY_E_UNSUPPORTED under Uniform / Adaptive, as that call. Normal and
 * depth have no consumer inside the library: they are films for the caller (external denoisers, compositing). */
int tray_render_first_hit_device(TrayDeviceScene* s, uint32_t tile_start, uint32_t tile_count, uint32_t spp, uint32_t sample_begin,
                                 uint32_t sample_end, uint64_t seed, float* albedo_dev, float* normal_dev, float* depth_dev, void* stream);

/* Render to a noise threshold: tiles [tile_start, tile_start+tile_count) of the max_spp-sample LowDiscrepancy frame, each tile sampled until
 * its estimated error drops below `threshold` (tile_count == 0 selects the whole queue, as in tray_render_tiles_device).
 * - Rounds. Round 0 renders the samples [0, min_spp) of every tile; round r >= 1 renders [min_spp 2^(r-1), min_spp 2^r) of the tiles that are
 *   still active. Each tile t ends with a power-of-two prefix [0, n_t) of its samples, min_spp <= n_t <= max_spp. Sample s is the sample the
 *   whole frame traces at s (tray_render_samples_device).
 * - Films. A round's range [a, b) is split at m = (a + b) / 2: [a, m) is added into even_dev, [m, b) into odd_dev, both RGBW films in the
 *   get_renderf32 layout that the caller zeroes beforehand. The image is even + odd: exactly the film of the samples [0, n_t) of every tile.
 * - Error of a tile, after every round, from the two films: for each of its pixels inside the image, with E / O the pixel of even / odd,
 *   e = E.rgb / E.w, o = O.rgb / O.w, d = (|e.r - o.r| + |e.g - o.g| + |e.b - o.b|) / 2, m = max(0, (sum(e) + sum(o)) / 2) and
 *   err_p = d / (1e-4 + sqrt(m)); a pixel with E.w <= 0 or O.w <= 0 counts as +inf. The tile's error is the maximum over its pixels (NaN if
 *   any pixel's is NaN): the two-buffer estimate of production renderers, relative to the square root of the pixel's brightness.
 * - Stopping rule. A tile stays active while !(error < threshold) and n_t < max_spp: a NaN error keeps it active.
 * - Outputs. tile_samples[i] / tile_error[i] (host arrays of tile_count entries, queue order) receive n_t and the tile's last error: the one
 *   of the round it stopped in. Later rounds of its neighbours still add samples to its edge pixels (the reconstruction filter's footprint),
 *   so that error is the metric of the returned films wherever no neighbouring tile took more samples.
 *   TrayKernelTiming covers the whole call: the samples of all rounds, every launch, render_ms from its first to its last event. The call
 *   synchronises on `stream` once per round (it reads the number of active tiles) and returns when it is done.
 * - Border pixels. The reconstruction filter reaches across tile borders. With a filter that has negative lobes (Mitchell-Netravali), a
 *   pixel next to tiles that ended with many times its tile's samples can get a total weight w near zero or below it, so that rgb / w
 *   resolves to black or to a saturated value; a uniform render has no such pixel. tray_scene_set_noise_ratio (below) bounds the ratio of n_t
 *   between neighbouring tiles, which keeps every pixel's own samples dominant; it is off by default, and without it callers should treat
 *   pixels with w <= 0, or with rgb / w far outside the image's range, as missing ("Rendering to a noise threshold": measured counts).
 * - Determinism. The films are sums of float atomics, so a tile whose error lies within rounding of `threshold` may be decided either way
 *   from one run to the next. What the call returns is always the film of exactly the reported [0, n_t) of every tile.
 * Returns TRAY_E_INVALID unless 2 <= min_spp <= max_spp are powers of two, threshold >= 0 (not NaN), no pointer is null and the two films are
 * different buffers; TRAY_E_UNSUPPORTED while tray_scene_set_sampler has chosen Uniform or Adaptive. */
int tray_render_noise_target_device(TrayDeviceScene* s, uint32_t tile_start, uint32_t tile_count, uint32_t min_spp, uint32_t max_spp,
                                    float threshold, uint64_t seed, float* even_dev, float* odd_dev, uint32_t* tile_samples,
                                    float* tile_error, void* stream);

/* Neighbour bound of the two noise-target calls (tray_render_noise_target_device, tray_render_noise_target_filtered_device): with max_ratio R,
 * 0 (off, the default) or a power of two in [2, 65536], neighbouring tiles end with sample counts at most R apart, max(n) <= R min(n).
 * - Neighbours. A tile's neighbours are the up to eight tiles around it in the grid of 8 x 8 tiles that belong to the call's range
 *   [tile_start, tile_start + tile_count). Tiles outside the range never render and do not count.
 * - Per-tile state. Every tile carries its own n_t: min_spp after round 0. Whenever a tile renders a round it renders its own next doubling
 *   [n_t, 2 n_t), split at 1.5 n_t into even and odd as above; tiles of different n_t may render in the same round.
 * - After a round's errors are taken, the set that renders the next round is the least set S such that
 *   (a) S holds every tile the stopping rule keeps: !(error < threshold) and n_t < max_spp; and
 *   (b) S holds every tile t with n_t < max_spp that has a neighbour u with n_u' > R n_t, where n_u' = 2 n_u if u is in S and n_u otherwise.
 *   (b) is a fixed point -- a pulled tile can pull its own neighbours --; the least one is unique, so S does not depend on an order of evaluation.
 * - A pulled tile's error is measured after its round like any tile's, and the stopping rule applies to it: tile_error stays the error of the
 *   last round the tile rendered. Within a round the tiles render and are measured by n_t, the smallest first, each group's error from the
 *   films as they stand when it is taken. The rounds end when S is empty.
 * - At the end the films are exactly the film of [0, n_t) of every tile, and max(n) <= R min(n) for every pair of neighbouring tiles.
 * - Cost. A bounded round reads one count per value of n_t (still one synchronisation per round) and launches one pair of renders and one
 *   error step per value of n_t that has tiles, log2(max_spp / min_spp) pull steps and up to as many list compactions. max_spp is at most
 *   32768 min_spp under a bound (16 values of n_t; TRAY_E_INVALID from the render call otherwise, before any device call).
 * - R = 0 is the call without the bound: the same launches in the same order, the same bits.
 * The setting belongs to the handle, as tray_scene_set_sampler's: it stays across tray_scene_update_frame and is read by both calls. Returns
 * TRAY_E_INVALID for a null scene or any other value. */
int tray_scene_set_noise_ratio(TrayDeviceScene* s, uint32_t max_ratio);

/* Denoise a frame rendered as two half films (tray_render_noise_target_device's even / odd, or two sample ranges of equal size from
 * tray_render_samples_device): dual-buffer non-local means (Rousselle, Knaus, Zwicker 2012). The difference of the halves estimates the noise
 * per pixel, and each half is filtered with weights computed from the OTHER half, so that the noise does not pick its own weights. A function
 * of two films: no scene handle. All arithmetic in f32, unfused; eps = 1e-7; sums over image positions skip positions outside the image.
 * - Resolve. With E / O the pixel p of even_dev / odd_dev (RGBW, get_renderf32 layout): valid(p) = E.w > 0 and O.w > 0 and every component of
 *   E and O is finite; a(p) = E.rgb / E.w, b(p) = O.rgb / O.w where valid, else 0.
 * - Noise estimate. v_c(p) = (a_c - b_c)^2 / 2 per channel c (the variance of one half, estimated from the two); V_c(p) = the mean of v_c over
 *   the valid pixels of the 3 x 3 box around p (0 if there is none). The halves of one low-discrepancy sequence are not independent; the
 *   estimate is used as it is.
 * - Distance of p and q = p + o, o in [-radius, radius]^2, in buffer x (a or b): with N(p, q) = the patch offsets n in [-patch, patch]^2 for
 *   which p + n and q + n are both inside the image and valid,
 *     t(p', q') = sum_c ((x_c(p') - x_c(q'))^2 - (V_c(p') + min(V_c(p'), V_c(q')))) / (eps + k^2 (V_c(p') + V_c(q'))),
 *     d2_x(p, q) = sum_{n in N} t(p + n, q + n) / (3 |N|).
 * - Weight. w_x(p, q) = exp(-max(0, d2_x(p, q))) if q is inside the image, valid and |N| > 0, else 0.
 * - Cross filtering. A(p) = sum_q w_b(p, q) a(q) / sum_q w_b(p, q), B(p) likewise with w_a and b; a quotient whose denominator is 0 is 0.
 *   out(p) = ((A + B) / 2, 1): an RGBW pixel of weight 1, which tray_resolve_srgb8 resolves like any film.
 * - Missing pixels. An invalid p (the border pixels of a noise-target film whose weight ended <= 0, above) is left out of every patch,
 *   contributes to nobody, and receives the weighted mean of its window like any pixel: the filter fills it from its neighbourhood.
 * - Every output channel lies between the minimum and the maximum of that channel of a and b over the valid pixels of the pixel's window, up
 *   to rounding. The order of the sums is the implementation's (a patch is summed separably); no atomics: the same bits in every run.
 * tray_denoise_scratch_bytes: the bytes of device scratch tray_denoise_device needs for a width x height film (0 if width or height is 0).
 * tray_denoise_device: out_dev = the filter of even_dev / odd_dev, in three kernel launches on `stream`, asynchronous, on the current device
 * (tray_init). Returns TRAY_E_INVALID unless width, height >= 1, 1 <= radius <= 10, patch <= 3, k > 0 and finite, no pointer is null, out_dev
 * differs from both films and the films from each other, and all four buffers are 16-byte aligned (hipMalloc's are). */
#define TRAY_DENOISE_RADIUS 7
#define TRAY_DENOISE_PATCH 3
#define TRAY_DENOISE_K 0.45f
uint64_t tray_denoise_scratch_bytes(uint32_t width, uint32_t height);
int tray_denoise_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev, uint32_t radius, uint32_t patch, float k,
                        float* out_dev, void* scratch_dev, void* stream);

/* tray_denoise_device for a frame of a sequence: the filter also searches the half films of N neighbouring frames. The sampler is keyed by the
 * frame, so the neighbours carry independent noise over almost the same image; NL-means matches patches, so no motion vectors are needed, and
 * where the motion is too fast for a neighbour's patches to match, its weights vanish and the frame is filtered as by tray_denoise_device.
 * - Frames. Frame 0 is the centre pair (E_0, O_0) = (even_dev, odd_dev); frames 1 ... N are (nb_even_dev[j - 1], nb_odd_dev[j - 1]), in the
 *   caller's order. Every frame j is resolved as above, on its own, into a_j, b_j, valid_j and V_j.
 * - Window. q runs over p + [-radius, radius]^2 in frame 0 and over p + [-radius_t, radius_t]^2 in every frame j >= 1.
 * - Distance of p (frame 0) and q (frame j) in buffer x: t takes the centre frame's values at p' = p + n, x_0(p') and V_0(p'), and frame j's at
 *   q' = q + n, x_j(q') and V_j(q'); pair(n) = valid_0(p') valid_j(q') (0 outside the image);
 *     d2_x(p, q, j) = sum_n t(p', q') pair(n) / (3 sum_n pair(n)) over the (2 patch + 1)^2 offsets n.
 * - Weight. w_x(p, q, j) = exp(-max(0, d2_x)) if q is inside the image, valid in frame j and sum_n pair(n) > 0, else 0.
 * - Cross filtering. A(p) = sum_j sum_q w_b(p, q, j) a_j(q) / sum_j sum_q w_b(p, q, j), B(p) likewise with w_a and b_j; a quotient whose
 *   denominator is 0 is 0. out(p) = ((A + B) / 2, 1).
 * - Order. The sums run over frame 0 first, then frames 1 ... N in the given order; within a frame dy outer and dx inner, ascending; f32,
 *   unfused, IEEE division, the library's own expf. With N = 0 the output is tray_denoise_device's, bit for bit. No atomics: the same bits in
 *   every run.
 * - Every output channel lies between the minimum and the maximum of that channel of a_j and b_j over the valid pixels of the pixel's windows
 *   in all frames, up to rounding.
 * tray_denoise_temporal_scratch_bytes: 128 bytes per pixel, whatever N is (the centre's records, the current neighbour's, the sums; 0 if width
 * or height is 0). nb_even_dev / nb_odd_dev are HOST arrays of n_neighbours device pointers, read during the call; they may be null only when
 * n_neighbours is 0. 3 (N + 1) kernel launches on `stream` (per frame tray_denoise_device's two preparing ones and one pass over the 32 x 16
 * tiles), asynchronous, no host synchronisation, on the current device (tray_init).
 * Returns TRAY_E_INVALID, before any device call, under tray_denoise_device's rules for width, height, radius, patch and k, unless
 * 1 <= radius_t <= radius and n_neighbours <= TRAY_DENOISE_MAX_NEIGHBOURS, if a film, out_dev or scratch_dev is null, or unless all 2 (N + 1)
 * films, out_dev and scratch_dev are pairwise different buffers, 16-byte aligned. */
#define TRAY_DENOISE_RADIUS_T 3
#define TRAY_DENOISE_MAX_NEIGHBOURS 8
uint64_t tray_denoise_temporal_scratch_bytes(uint32_t width, uint32_t height);
int tray_denoise_temporal_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev, uint32_t n_neighbours,
                                 const float* const* nb_even_dev, const float* const* nb_odd_dev, uint32_t radius, uint32_t radius_t, uint32_t patch,
                                 float k, float* out_dev, void* scratch_dev, void* stream);

/* The two cross-filtered halves of tray_denoise_device's statement as RGBW films: fa = (A(p), wA), fb = (B(p), wB), where wA = 1 if A's denominator
 * sum_q w_b(p, q) is > 0, else 0 (then A = 0), wB likewise. (fa.rgb + fb.rgb) * 0.5f is tray_denoise_device's out.rgb, bit for bit.
 * |fa - fb| / 2 is a per-pixel confidence map of the denoised frame: the two halves are two estimates of the same image.
 * blocks_dev: null = every pixel; else n_blocks indices (row-major, tiles_x = ceil(width / 32)) of 32 x 16 pixel blocks: only those are computed and
 * written, every other pixel of fa / fb is left as it is. An index outside the frame's blocks is passed over. n_blocks == 0 with a list is valid
 * and launches nothing; with a null list n_blocks is not read.
 * The argument rules are tray_denoise_device's and the scratch size is tray_denoise_scratch_bytes; the two films, the two outputs and the scratch
 * must be five different buffers, 16-byte aligned; a list longer than the frame has blocks is TRAY_E_INVALID. Three launches on `stream`
 * (tray_denoise_device's two preparing ones and the filter), asynchronous, on the current device. No atomics: the same bits in every run. */
#define TRAY_DENOISE_BLOCK_W 32
#define TRAY_DENOISE_BLOCK_H 16
int tray_denoise_halves_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev, uint32_t radius, uint32_t patch, float k,
                               const uint32_t* blocks_dev, uint32_t n_blocks, float* fa_dev, float* fb_dev, void* scratch_dev, void* stream);

/* tray_denoise_device with the weights measured on another pair of films: the patch distances come from the guide (GA, GB) = (guide_a_dev,
 * guide_b_dev), the averaged colours from the values (even_dev, odd_dev). A guide with less noise than the values (a first pass's output)
 * picks better weights than the values themselves can.
 * - Values. a, b and valid are resolved from (even_dev, odd_dev) as tray_denoise_device resolves them.
 * - Guide. ga = GA.rgb / GA.w, gb = GB.rgb / GB.w and gvalid by the same rule applied to (GA, GB): both weights > 0 and all eight words finite;
 *   else ga = gb = 0. Vg = the 3 x 3 mean of (ga - gb)^2 / 2 over the gvalid pixels of the box (0 if there is none). The films of
 *   tray_denoise_halves_device (weight 1 or 0) are valid guides as they stand.
 * - Distance of p and q = p + o in guide buffer x (ga or gb): t(p', q') as in tray_denoise_device from x(p'), x(q'), Vg(p'), Vg(q');
 *   pair(n) = gvalid(p') gvalid(q') (0 outside the image); d2_x(p, q) = sum_n t(p', q') pair(n) / (3 sum_n pair(n)) over the (2 patch + 1)^2
 *   offsets n, p' = p + n, q' = q + n.
 * - Weight. w_x(p, q) = exp(-max(0, d2_x)) if q is inside the image, valid(q) holds (the VALUES' validity) and sum_n pair(n) > 0, else 0.
 * - Output. A(p) = sum_q w_gb(p, q) a(q) / sum_q w_gb(p, q), B(p) = sum_q w_ga(p, q) b(q) / sum_q w_ga(p, q); a quotient whose denominator is 0
 *   is 0. out(p) = ((A + B) / 2, 1). A pixel that is invalid in the values and valid in the guide takes part in patches and is filled from its
 *   window.
 * - Order. dy outer, dx inner, ascending; f32, unfused, IEEE division, the library's own expf. No atomics: the same bits in every run. With
 *   guide_a_dev == even_dev and guide_b_dev == odd_dev the output is tray_denoise_device's, bit for bit; the guide may alias the films for that.
 * - Every output channel lies between the minimum and the maximum of that channel of a and b over the valid pixels of the pixel's window, up
 *   to rounding: the guide only chooses weights.
 * tray_denoise_guided_scratch_bytes: 96 bytes per pixel (the values' records and the guide's, 48 each; 0 if width or height is 0).
 * tray_denoise_guided_device: five kernel launches on `stream` (tray_denoise_device's two preparing ones for the values, the same two for the
 * guide, one filter over the 32 x 16 tiles), asynchronous, no host synchronisation, on the current device (tray_init).
 * Returns TRAY_E_INVALID, before any device call, under tray_denoise_device's rules for width, height, radius, patch and k, if a pointer is
 * null, if even_dev == odd_dev or guide_a_dev == guide_b_dev, unless out_dev and scratch_dev differ from all four films and from each other,
 * or unless all six buffers are 16-byte aligned. */
uint64_t tray_denoise_guided_scratch_bytes(uint32_t width, uint32_t height);
int tray_denoise_guided_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev, const float* guide_a_dev,
                               const float* guide_b_dev, uint32_t radius, uint32_t patch, float k, float* out_dev, void* scratch_dev, void* stream);

/* Two-pass NL-means: the second pass measures its patch distances on the first pass's output and averages the original films. By definition
 * tray_denoise_halves_device(even_dev, odd_dev, radius, patch, k, blocks_dev = null) into (fa, fb), followed by
 * tray_denoise_guided_device(even_dev, odd_dev, fa, fb, radius2, patch2, k2): the output is what those two calls give, bit for bit.
 * tray_denoise_two_pass_scratch_bytes: 128 bytes per pixel (0 if width or height is 0), laid out as: the films' records, 48 bytes per pixel (the
 * first pass's scratch, read again as the second pass's values); fa and fb, 16 each; the records of (fa, fb), 48.
 * Six kernel launches on `stream`, in this order: the two preparing ones for the films, the first pass's filter (the halves) over the 32 x 16
 * tiles, the two preparing ones for (fa, fb), the guided filter; asynchronous, no host synchronisation, on the current device (tray_init).
 * Returns TRAY_E_INVALID, before any device call, under tray_denoise_device's rules for width, height and each of (radius, patch, k) and
 * (radius2, patch2, k2), if a pointer is null, or unless the two films, out_dev and scratch_dev are four different buffers, 16-byte aligned. */
#define TRAY_DENOISE_RADIUS2 5
#define TRAY_DENOISE_PATCH2 1
#define TRAY_DENOISE_K2 1.0f
uint64_t tray_denoise_two_pass_scratch_bytes(uint32_t width, uint32_t height);
int tray_denoise_two_pass_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev, uint32_t radius, uint32_t patch, float k,
                                 uint32_t radius2, uint32_t patch2, float k2, float* out_dev, void* scratch_dev, void* stream);

/* Albedo-demodulated denoising: the colour is divided by the first-hit albedo (tray_render_first_hit_device's film of the same frame), the
 * smooth remainder is filtered, and the texture is multiplied back in.
 * - With ALB the pixel of albedo_dev: s_c(p) = max(ALB_c / ALB.w, 0) + TRAY_DEMOD_EPS where ALB.w > 0 and all four words are finite, else
 *   s_c(p) = 1 (the resolved albedo goes slightly negative at texture edges under a filter with negative lobes: hence the max).
 * - E'(p) = (E.rgb / s, E.w), O' likewise. D = tray_denoise_device(E', O', radius, patch, k), or tray_denoise_two_pass_device(E', O', radius,
 *   patch, k, radius2, patch2, k2) when radius2 >= 1; radius2 == 0 means one pass. out = (D.rgb * s, 1). f32, unfused, IEEE division.
 * - An albedo film without a valid pixel gives the plain call's bits.
 * tray_denoise_demodulated_scratch_bytes: the filter's scratch (48 or 128 bytes per pixel) plus 32 for E' and O' behind it; 0 if width or
 * height is 0. Launches in stream order, no host synchronisation, on the current device: one that writes E' and O', the filter's three (or
 * six), one that scales out_dev in place: 5 or 8.
 * Returns TRAY_E_INVALID, before any device call, under tray_denoise_device's (and the two-pass call's) rules for the filter parameters and
 * the buffers, or if albedo_dev is null, equals another buffer or is not 16-byte aligned. */
#define TRAY_DEMOD_EPS 0.01f
uint64_t tray_denoise_demodulated_scratch_bytes(uint32_t width, uint32_t height, uint32_t radius2);
int tray_denoise_demodulated_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev, const float* albedo_dev,
                                    uint32_t radius, uint32_t patch, float k, uint32_t radius2, uint32_t patch2, float k2, float* out_dev,
                                    void* scratch_dev, void* stream);

/* tray_denoise_temporal_device on albedo-demodulated films: every frame's colour is divided by that frame's own first-hit albedo, the smooth
 * remainders are filtered together, and the centre frame's texture is multiplied back in. Where the texture itself changes from frame to frame
 * (an animated image, a moving textured object) a neighbour's colour patches do not match the centre's, while the remainders do.
 * - Frames as in tray_denoise_temporal_device; frame j (0 = the centre) also has an albedo film ALB_j: albedo_dev, nb_albedo_dev[j - 1].
 * - Scale. s_j(p) from ALB_j by tray_denoise_demodulated_device's rule: max(ALB_c / ALB.w, 0) + TRAY_DEMOD_EPS where ALB.w > 0 and all four
 *   words are finite, else 1.
 * - Demodulated films. E'_j = (E_j.rgb / s_j, E_j.w), O'_j likewise. A pixel of frame j is valid by tray_denoise_device's rule applied to
 *   E'_j and O'_j: both weights > 0 and all eight words of the QUOTIENTS finite.
 * - Filter. D = tray_denoise_temporal_device(E'_0, O'_0, N, E'_1 ..., O'_1 ..., radius, radius_t, patch, k).
 * - Output. out = (D.rgb * s_0, 1). f32, unfused, IEEE division. No atomics: the same bits in every run.
 * - With N = 0 the output is tray_denoise_demodulated_device's with radius2 = 0, bit for bit; with albedo films without a valid pixel it is
 *   tray_denoise_temporal_device's (x / 1 and x * 1 are exact); in general it is the output of the three steps above made one after the other.
 * tray_denoise_temporal_demodulated_scratch_bytes: tray_denoise_temporal_scratch_bytes, 128 bytes per pixel whatever N is, laid out as there
 * (0 if width or height is 0): E' and O' are never written to memory. nb_even_dev / nb_odd_dev / nb_albedo_dev are HOST arrays of
 * n_neighbours device pointers, read during the call; they may be null only when n_neighbours is 0. 3 (N + 1) kernel launches on `stream`
 * (per frame one that resolves the demodulated films, tray_denoise_device's second preparing one, and one pass over the 32 x 16 tiles, the last
 * of which scales its output), asynchronous, no host synchronisation, on the current device (tray_init).
 * Returns TRAY_E_INVALID, before any device call, under tray_denoise_temporal_device's rules, if an albedo film is null, or unless all
 * 3 (N + 1) films, out_dev and scratch_dev are pairwise different buffers, 16-byte aligned. */
uint64_t tray_denoise_temporal_demodulated_scratch_bytes(uint32_t width, uint32_t height);
int tray_denoise_temporal_demodulated_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev, const float* albedo_dev,
                                             uint32_t n_neighbours, const float* const* nb_even_dev, const float* const* nb_odd_dev,
                                             const float* const* nb_albedo_dev, uint32_t radius, uint32_t radius_t, uint32_t patch, float k,
                                             float* out_dev, void* scratch_dev, void* stream);

/* Two-pass temporal NL-means: a second pass over ALL frames whose weights are measured on first-pass output. Three calls; the third is defined
 * by the first two and by tray_denoise_halves_device.
 *
 * tray_denoise_temporal_halves_device: the two cross-filtered halves of tray_denoise_temporal_device's statement as RGBW films, in
 * tray_denoise_halves_device's convention: fa = (A(p), wA), fb = (B(p), wB) with A, B the quotients of that statement over all frames' windows,
 * wA = 1 if A's denominator sum_j sum_q w_b(p, q, j) is > 0, else 0 (then A = 0), wB likewise. The arguments are tray_denoise_temporal_device's
 * with fa_dev, fb_dev in place of out_dev. (fa.rgb + fb.rgb) * 0.5f is tray_denoise_temporal_device's out.rgb, bit for bit; with N = 0 the
 * films are tray_denoise_halves_device's with blocks_dev = null, bit for bit. No atomics: the same bits in every run.
 * tray_denoise_temporal_halves_scratch_bytes: 128 bytes per pixel whatever N is, laid out as tray_denoise_temporal_device's (the centre's
 * records, 48; the current neighbour's, 48; the sums between passes, 32; 0 if width or height is 0). 3 (N + 1) kernel launches on `stream`:
 * per frame, the centre first, tray_denoise_device's two preparing ones and one pass over the 32 x 16 tiles, the last of which stores the halves.
 *
 * tray_denoise_temporal_guided_device: tray_denoise_temporal_device with the weights measured on guides, as tray_denoise_guided_device measures
 * them. Frame j (0 = the centre; frames 1 ... N in the caller's order) has values (E_j, O_j) = (even_dev, odd_dev) / (nb_even_dev[j - 1],
 * nb_odd_dev[j - 1]) and a guide (GA_j, GB_j) = (guide_a_dev, guide_b_dev) / (nb_guide_a_dev[j - 1], nb_guide_b_dev[j - 1]).
 * - Values. a_j, b_j and valid_j are resolved from (E_j, O_j) as tray_denoise_device resolves them.
 * - Guides. ga_j, gb_j, gvalid_j and Vg_j are resolved from (GA_j, GB_j), each frame on its own, as tray_denoise_guided_device resolves its guide.
 * - Window and order. As tray_denoise_temporal_device: q runs over p + [-radius, radius]^2 in frame 0 and over p + [-radius_t, radius_t]^2 in
 *   every frame j >= 1; the sums run over frame 0 first, then frames 1 ... N in the given order; within a frame dy outer and dx inner, ascending.
 * - Distance of p (frame 0) and q (frame j) in guide buffer x (ga or gb): t(p', q') as in tray_denoise_device from x_0(p'), Vg_0(p'), x_j(q'),
 *   Vg_j(q'); pair(n) = gvalid_0(p') gvalid_j(q') (0 outside the image); d2_x(p, q, j) = sum_n t(p', q') pair(n) / (3 sum_n pair(n)) over the
 *   (2 patch + 1)^2 offsets n, p' = p + n, q' = q + n.
 * - Weight. w_x(p, q, j) = exp(-max(0, d2_x)) if q is inside the image, valid_j(q) holds (the VALUES' validity) and sum_n pair(n) > 0, else 0.
 * - Output. A(p) = sum_j sum_q w_gb(p, q, j) a_j(q) / sum_j sum_q w_gb(p, q, j), B(p) likewise with w_ga and b_j; a quotient whose denominator
 *   is 0 is 0. out(p) = ((A + B) / 2, 1).
 * - Arithmetic. f32, unfused, IEEE division, the library's own expf. No atomics: the same bits in every run.
 * - Identities, to the bit: (i) with every frame's guide equal to its values (guide_a_dev == even_dev, guide_b_dev == odd_dev,
 *   nb_guide_a_dev[j] == nb_even_dev[j], nb_guide_b_dev[j] == nb_odd_dev[j]; the guides may alias the films for that) the output is
 *   tray_denoise_temporal_device's; (ii) with N = 0 it is tray_denoise_guided_device's.
 * - Every output channel lies between the minimum and the maximum of that channel of a_j and b_j over the valid pixels of the pixel's windows
 *   in all frames, up to rounding: the guides only choose weights.
 * tray_denoise_temporal_guided_scratch_bytes: 176 bytes per pixel whatever N is (0 if width or height is 0), laid out as: the records of the
 * centre's guide, 48 bytes per pixel; the records of the current neighbour's guide, 48; the records of the current frame's values, 48; the sums
 * between passes, 32. 5 (N + 1) kernel launches on `stream`: per frame, the centre first, the two preparing ones for the frame's values, the
 * same two for its guide, one pass over the 32 x 16 tiles.
 *
 * tray_denoise_temporal_two_pass_device: by definition
 *   (fa_0, fb_0) = tray_denoise_temporal_halves_device(all frames, radius, radius_t, patch, k),
 *   (fa_j, fb_j) = tray_denoise_halves_device(E_j, O_j, radius, patch, k, blocks_dev = null) for every neighbour j = 1 ... N,
 *   out = tray_denoise_temporal_guided_device(values: the frames, guides: (fa_j, fb_j), radius2, radius_t2, patch2, k2):
 * the centre is guided by its pilot over all frames, every neighbour by its own single-frame pilot. The output is what those calls give, bit
 * for bit; with N = 0 it is tray_denoise_two_pass_device's, bit for bit.
 * tray_denoise_temporal_two_pass_scratch_bytes: 256 bytes per pixel whatever N is (0 if width or height is 0), laid out as: the centre's
 * records, 48 bytes per pixel (the first pass's, read again as the second pass's values of frame 0); the current neighbour's records, 48; the
 * sums between passes, 32 (the first pass's, then the second's); fa and fb of the frame in hand, 16 each; the records of the centre's pilot,
 * 48; the records of the current neighbour's pilot, 48. The neighbours are processed one at a time, so a neighbour's films are resolved once
 * in each pass. 9 N + 6 kernel launches on `stream`, in this order: the 3 (N + 1) of tray_denoise_temporal_halves_device; the two preparing
 * ones for (fa_0, fb_0) and the centre's guided pass; then per neighbour, in the caller's order, the two preparing ones for its films, its
 * first-pass filter (the halves) over the 32 x 16 tiles, the two preparing ones for (fa_j, fb_j), its guided pass.
 *
 * All three: nb_* are HOST arrays of n_neighbours device pointers, read during the call; they may be null only when n_neighbours is 0. Every
 * launch runs on `stream`, asynchronous, no host synchronisation, on the current device (tray_init).
 * Return TRAY_E_INVALID, before any device call, under tray_denoise_temporal_device's rules for width, height, (radius, radius_t, patch, k)
 * and n_neighbours; the two-pass call likewise for (radius2, radius_t2, patch2, k2): 1 <= radius_t2 <= radius2 <= 10, patch2 <= 3, k2 > 0 and
 * finite; if a film, an output or scratch_dev is null; unless every buffer is 16-byte aligned; unless the outputs and scratch_dev differ from
 * every film and from each other; if the two films of a pair (a frame's values, a frame's guide) are one buffer. In the halves and the
 * two-pass call all 2 (N + 1) films are pairwise different, as in tray_denoise_temporal_device; in the guided call the films are only read and
 * a guide may be its own frame's values. */
#define TRAY_DENOISE_RADIUS_T2 3
uint64_t tray_denoise_temporal_halves_scratch_bytes(uint32_t width, uint32_t height);
int tray_denoise_temporal_halves_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev, uint32_t n_neighbours,
                                        const float* const* nb_even_dev, const float* const* nb_odd_dev, uint32_t radius, uint32_t radius_t,
                                        uint32_t patch, float k, float* fa_dev, float* fb_dev, void* scratch_dev, void* stream);
uint64_t tray_denoise_temporal_guided_scratch_bytes(uint32_t width, uint32_t height);
int tray_denoise_temporal_guided_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev, const float* guide_a_dev,
                                        const float* guide_b_dev, uint32_t n_neighbours, const float* const* nb_even_dev,
                                        const float* const* nb_odd_dev, const float* const* nb_guide_a_dev, const float* const* nb_guide_b_dev,
                                        uint32_t radius, uint32_t radius_t, uint32_t patch, float k, float* out_dev, void* scratch_dev, void* stream);
uint64_t tray_denoise_temporal_two_pass_scratch_bytes(uint32_t width, uint32_t height);
int tray_denoise_temporal_two_pass_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev, uint32_t n_neighbours,
                                          const float* const* nb_even_dev, const float* const* nb_odd_dev, uint32_t radius, uint32_t radius_t,
                                          uint32_t patch, float k, uint32_t radius2, uint32_t radius_t2, uint32_t patch2, float k2, float* out_dev,
                                          void* scratch_dev, void* stream);

/* The two-pass temporal filter on albedo-demodulated films: the three calls above in the domain of tray_denoise_temporal_demodulated_device.
 * Frame j (0 = the centre) has values (E_j, O_j) and an albedo film ALB_j (albedo_dev, nb_albedo_dev[j - 1]); s_j and the demodulated films
 * E'_j = (E_j.rgb / s_j, E_j.w), O'_j likewise, are those of tray_denoise_temporal_demodulated_device; E' and O' are never written to memory.
 *
 * tray_denoise_temporal_demodulated_halves_device: (fa, fb) = tray_denoise_temporal_halves_device(E'_0, O'_0, N, E'_1 ..., O'_1 ..., radius,
 * radius_t, patch, k), bit for bit. The halves are NOT multiplied by s_0: they are guides and stay in the domain the second pass measures in.
 * With N = 0 they are a frame's own single-frame halves in that domain. 128 bytes of scratch per pixel and 3 (N + 1) launches, as there.
 *
 * tray_denoise_temporal_demodulated_guided_device: D = tray_denoise_temporal_guided_device(values (E'_j, O'_j), guides (GA_j, GB_j) as the
 * caller gives them -- already in the demodulated domain, e.g. the halves call's films --, radius, radius_t, patch, k); out = (D.rgb * s_0, 1),
 * bit for bit. 176 bytes of scratch per pixel and 5 (N + 1) launches, as there.
 *
 * tray_denoise_temporal_demodulated_two_pass_device: by definition D = tray_denoise_temporal_two_pass_device(E'_0, O'_0, N, E'_1 ..., O'_1 ...,
 * radius, radius_t, patch, k, radius2, radius_t2, patch2, k2) and out = (D.rgb * s_0, 1); the output is what those three steps give one after
 * the other, bit for bit. It is also the guided call above with the guides (fa_0, fb_0) = the halves call above over all frames and (fa_j, fb_j)
 * = the halves call above of frame j alone (N = 0), bit for bit. With N = 0 it is tray_denoise_demodulated_device's output with radius2 >= 1;
 * with albedo films without a valid pixel it is tray_denoise_temporal_two_pass_device's (x / 1 and x * 1 are exact). 256 bytes of scratch per
 * pixel, laid out as there, and 9 N + 6 launches in that call's order: the demodulation is folded into the first preparing launch of every
 * frame's films, the remodulation into the store of the last guided pass.
 *
 * All three: f32, unfused, IEEE division, no atomics: the same bits in every run. The *_scratch_bytes functions return 0 if width or height
 * is 0. nb_* are HOST arrays of n_neighbours device pointers, read during the call; they may be null only when n_neighbours is 0. Every launch
 * runs on `stream`, asynchronous, no host synchronisation, on the current device (tray_init).
 * Return TRAY_E_INVALID, before any device call, under the rules of the call of the same name without `_demodulated` for width, height, the
 * filter parameters and n_neighbours; if a film, an albedo film, an output or scratch_dev is null; unless all films of all frames -- 3 (N + 1)
 * in the halves and the two-pass call, 5 (N + 1) in the guided call, whose guides may NOT alias the values --, the outputs and scratch_dev are
 * pairwise different buffers, 16-byte aligned. */
uint64_t tray_denoise_temporal_demodulated_halves_scratch_bytes(uint32_t width, uint32_t height);
int tray_denoise_temporal_demodulated_halves_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev,
                                                    const float* albedo_dev, uint32_t n_neighbours, const float* const* nb_even_dev,
                                                    const float* const* nb_odd_dev, const float* const* nb_albedo_dev, uint32_t radius,
                                                    uint32_t radius_t, uint32_t patch, float k, float* fa_dev, float* fb_dev, void* scratch_dev,
                                                    void* stream);
uint64_t tray_denoise_temporal_demodulated_guided_scratch_bytes(uint32_t width, uint32_t height);
int tray_denoise_temporal_demodulated_guided_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev,
                                                    const float* albedo_dev, const float* guide_a_dev, const float* guide_b_dev, uint32_t n_neighbours,
                                                    const float* const* nb_even_dev, const float* const* nb_odd_dev,
                                                    const float* const* nb_albedo_dev, const float* const* nb_guide_a_dev,
                                                    const float* const* nb_guide_b_dev, uint32_t radius, uint32_t radius_t, uint32_t patch, float k,
                                                    float* out_dev, void* scratch_dev, void* stream);
uint64_t tray_denoise_temporal_demodulated_two_pass_scratch_bytes(uint32_t width, uint32_t height);
int tray_denoise_temporal_demodulated_two_pass_device(uint32_t width, uint32_t height, const float* even_dev, const float* odd_dev,
                                                      const float* albedo_dev, uint32_t n_neighbours, const float* const* nb_even_dev,
                                                      const float* const* nb_odd_dev, const float* const* nb_albedo_dev, uint32_t radius,
                                                      uint32_t radius_t, uint32_t patch, float k, uint32_t radius2, uint32_t radius_t2, uint32_t patch2,
                                                      float k2, float* out_dev, void* scratch_dev, void* stream);

/* tray_render_noise_target_device with the stopping rule on the image that will be shown: the rounds, the even / odd split, n_t, the outputs,
 * TrayKernelTiming and the error returns are that call's, word for word, and the films it returns are still the unfiltered films of exactly
 * [0, n_t) of every tile. One thing differs: the error of a tile in a round is that call's metric evaluated on (fa, fb) =
 * tray_denoise_halves_device(radius, patch, k) of the films as they stand after that round, in place of (even, odd): e = fa.rgb, o = fb.rgb, and
 * a pixel with wA = 0 or wB = 0 counts as +inf, as a pixel without weight does there. The difference of the filtered halves estimates the
 * residual error of the denoised image (Rousselle, Knaus, Zwicker 2012), so samples go where the filter cannot repair the noise. A border pixel
 * whose film weight ended <= 0 is filled by the filter and no longer keeps its tile sampling up to max_spp.
 * - Each round filters only the 32 x 16 blocks that hold an active tile (round 0: a tile of the selected range); the host reads the number of
 *   active tiles and of blocks in its one copy and synchronisation per round, plus one before round 0 for that round's block count.
 * - out_dev (may be null): with it the call ends with tray_denoise_device's three launches on the final films, inside the call's timing, so
 *   out_dev equals a separate tray_denoise_device call's output bit for bit.
 * - scratch_dev: tray_noise_target_filtered_scratch_bytes(width, height) bytes of the scene's film size (the filter's 48 bytes per pixel, fa
 *   and fb, the block flags, list and counts; 0 if width or height is 0). Its layout is private.
 * - Determinism is tray_render_noise_target_device's: the films are sums of float atomics, so a tile whose error lies within rounding of
 *   `threshold` may be decided either way from one run to the next; what is returned is always the film of exactly the reported [0, n_t).
 * - A stopped tile's reported error is that of the round it stopped in. Its filter window then still held its neighbours' earlier samples: the
 *   error is the metric of the halves of the returned films only for the tiles that were computed in the call's last round.
 * Returns TRAY_E_INVALID under tray_render_noise_target_device's rules and tray_denoise_device's for radius, patch and k, if scratch_dev is null,
 * or unless the films, the scratch and (if given) the output are different buffers, 16-byte aligned; TRAY_E_UNSUPPORTED as that call. */
uint64_t tray_noise_target_filtered_scratch_bytes(uint32_t width, uint32_t height);
int tray_render_noise_target_filtered_device(TrayDeviceScene* s, uint32_t tile_start, uint32_t tile_count, uint32_t min_spp, uint32_t max_spp,
                                             float threshold, uint64_t seed, float* even_dev, float* odd_dev, uint32_t radius, uint32_t patch, float k,
                                             float* out_dev /* may be null */, void* scratch_dev, uint32_t* tile_samples, float* tile_error,
                                             void* stream);

/* Host-side enumeration of the Morton-queue indices tray_render_shard_device renders for `shard`
 * (same mapping; lets callers and tests reason about the partition without a GPU). */
int tray_shard_tiles(uint32_t n_tiles, uint32_t shard, uint32_t n_shards, uint32_t chunk_tiles,
                     uint32_t* out, uint32_t cap, uint32_t* n_out);

/* Synchronous convenience wrapper: renders into a zeroed device buffer, adds it into rgbw_host
 * (host, width*height*4 f32) — semantics of film::Image::add_pixels. */
int tray_render_tiles(TrayDeviceScene* s, uint32_t tile_start, uint32_t tile_count,
                      uint32_t spp, uint64_t seed, float* rgbw_host);

/* ---- the other Samplers (src/sampler/mod.rs:20-49) -----------------------------------------------------------------
 * thread_work constructs `sampler::LowDiscrepancy::new(queue.block_dim(), spp)` (exec/multithreaded.rs:74); sampler/uniform.rs and
 * sampler/adaptive.rs implement the same trait and are what a maintainer would write there instead. tray_scene_set_sampler selects
 * which one the render calls on this handle stand for:
 *   TRAY_SAMPLER_LOW_DISCREPANCY  LowDiscrepancy::new(dim, spp) -- the default; `spp` of the render call (ld.rs:20-31)
 *   TRAY_SAMPLER_UNIFORM          Uniform::new(dim): one sample at the centre of every pixel, every other number an independent
 *                                 uniform draw (uniform.rs:22-47); the render call's spp is not used
 *   TRAY_SAMPLER_ADAPTIVE         Adaptive::new(dim, min_spp, max_spp): min_spp samples per pixel, then step_size more while the
 *                                 luminance of any of the pixel's samples so far lies more than 50 % off their running average and fewer
 *                                 than max_spp have been taken (adaptive.rs:34-75, 133-143 incl. its (i - 1) / i averaging and the
 *                                 sample-index offsets of adaptive.rs:112-121); min_spp / max_spp are rounded up to powers of two as
 *                                 Adaptive::new does (0 counts as 1); the render call's spp is not used
 * Every sample is still keyed by (seed, frame, pixel, pass, index) (TRAY-CBRNG), so shards and tile ranges add up
 * to the same film. Uniform and Adaptive run one thread per camera sample of a pass (k_sampler_pass) for every scene; the per-pixel
 * sample counts of the last render are reported through TrayKernelTiming.samples (their sum). min_spp / max_spp are ignored for the
 * other two kinds. Returns TRAY_E_INVALID for an unknown kind or max_spp < min_spp after rounding. */
enum { TRAY_SAMPLER_LOW_DISCREPANCY = 0, TRAY_SAMPLER_UNIFORM = 1, TRAY_SAMPLER_ADAPTIVE = 2 };
int tray_scene_set_sampler(TrayDeviceScene* s, uint32_t kind, uint32_t min_spp, uint32_t max_spp);
/* Adaptive::new's step_size (adaptive.rs:48): ((max_spp - min_spp) / 5).next_power_of_two(), of the ROUNDED min / max */
uint32_t tray_adaptive_step(uint32_t min_spp, uint32_t max_spp);

/* Timing of the most recent tray_render_tiles_device launch sequence on this scene, measured with
 * HIP events on the launch stream. Blocks until those kernels finished. */
typedef struct TrayKernelTiming {
    float render_ms;        /* k_path_tiles */
    uint32_t launches;
    uint64_t samples;       /* camera samples traced */
    uint64_t vertices;      /* path vertices shaded (iterations of path.rs:69) */
    uint64_t rays;          /* Scene::intersect calls of the reference's algorithm. A few of them are proven irrelevant before they are traced
                               -- a BSDF-sampled light ray that misses the light's own primitive, an occlusion ray whose BSDF value is
                               black -- and only counted */
    uint64_t retraced;      /* rays of the flat instance loop whose closest candidates tied (or sat inside one another's bounding-box
                             * window) and that were therefore traced again with the reference's BVH<Instance> traversal
                             * (geometry/bvh.rs:81-130), which decides by its visiting order; about 1 in 1e7 on cornell_box */
} TrayKernelTiming;
int tray_last_timing(TrayDeviceScene* s, TrayKernelTiming* t);

/* Footprint and shape of the wavefront schedule (scenes that traverse BVH<Instance>: more than 16 instances) -- the reference has no
 * counterpart: its workers keep one path per thread on the stack (exec/multithreaded.rs:72-114); here up to 32 M paths are in flight in a
 * pool in HBM. pool_slots: paths in flight (0 = the library's rule: 32 M, never more than 4096 per tile, the pool with its queues within a
 * third of the device's free memory, a moving scene's per-path transform cache within two fifths); views: independent halves / thirds /
 * quarters of the pool on streams of their own (0 = rule: 1 from 24 M slots, else 2); slices: work items a tile's samples are cut into
 * (0 = rule; a power of two <= 16). A host that keeps several device scenes on one GPU sets pool_slots so that they fit beside each other
 * (0.47 KB per slot + 112 B per slot and instance that moves within a frame). Takes effect at the next render call (the buffers are freed
 * and allocated anew if the pool's size changes). A launch of a moving scene that evaluates transforms per path (tray_scene_set_transform_table)
 * reads a per-path cache with a record for every pool slot: its pool is no larger than the cache's budget (the library's rule and
 * TRAYHIP_XF_CACHE_BYTES; this setting bounds the pool, not the cache), and a larger pool left by a launch that read the transform table gets a
 * cache allocated anew for all of its slots -- or, if that would take more than two fifths of the free memory, is allocated anew at the cache's
 * size. If an allocation fails the library halves the pool down to 16 384 slots before it returns TRAY_E_NOMEM, and the handle stays usable. The environment switches TRAYHIP_WF_SLOTS / _PIPES / _SLICES
 * (measurement only) override these. TRAY_E_INVALID for views > 4 or slices not a power of two <= 16. */
int tray_scene_set_wavefront(TrayDeviceScene* s, uint32_t pool_slots, uint32_t views, uint32_t slices);
/* The schedule the last render call on this scene ran with (what tools/pmc_workloads.py records beside its counters). */
typedef struct TrayScheduleInfo {
    uint32_t wavefront;           /* 1: the scene takes the wavefront schedule, 0: the tile kernel */
    uint32_t launched_wavefront;  /* 1: the last render call ran the wavefront schedule (0 also for the Uniform / Adaptive sampler passes) */
    uint32_t pool_slots, chunks;  /* paths in flight (0 until the first wavefront launch allocated the pool), chunks of 256 */
    uint32_t views, slices;       /* of the last wavefront launch */
    uint32_t n_moving;            /* instances that move within the frame (columns of the per-path transform cache) */
    uint32_t tile_workgroups;     /* persistent workgroups of the tile kernel */
    uint64_t pool_bytes, schedule_bytes, xf_cache_bytes;   /* pool alone; pool + queues + bins; per-path transform cache */
    uint32_t transform_table;     /* 1: the last launch read the frame's transform table (tray_scene_set_transform_table) */
    uint32_t binned_stages;       /* wavefront schedule: traversal stages whose rays are sorted by (origin cell, direction octant) before they are
                                   * traced -- bit 0: camera / continuation rays, bit 1: occlusion rays (round 6; this word was padding before) */
    uint64_t xf_table_bytes;                               /* the transform table's buffer, if there is one: sized once for every instance that any frame of the sequence can move */
} TrayScheduleInfo;
int tray_last_schedule(TrayDeviceScene* s, TrayScheduleInfo* out);

/* Moving scenes: where a path's AnimatedTransform::transform(ray.time) comes from (linalg/animated_transform.rs:40-56; the reference
 * rebuilds it at every instance visit, geometry/receiver.rs:30). A camera sample's shutter time is one of 2^24 values (sampler/ld.rs:100-104),
 * every ray of the path inherits it (path.rs:110), so the transform is a function of a 24-bit index. mode 1: build, per frame and on the
 * first launch, the TABLE of every moving instance's (and a moving camera's) transform at all 2^24 times -- 2.1 GB each (128-byte records), ~1.5 ms each to
 * build, the same evaluation at the same times: the same bits -- and read it; mode 0: evaluate per camera sample into a per-path cache
 * (128 B per path and instance); mode -1 (default): the table for launches of >= 3e7 camera samples (a 1080p frame at 16 spp: each index is needed about twice or more),
 * for every later launch of the frame once it exists, and for the frames that follow it through tray_scene_update_frame (the buffer -- sized once for every
 * instance whose transform has several keyframes -- and the wavefront pool are handed on). If the table cannot be allocated the per-path cache serves, and vice versa.
 * TRAYHIP_XF_TABLE=0|1 (measurement) overrides. tray_debug_transform_table compares n pseudo-random records of the frame's table with a fresh
 * evaluation, bit for bit, and reports how many differ (test hook; TRAY_E_INVALID if the frame has no table yet). */
int tray_scene_set_transform_table(TrayDeviceScene* s, int mode);
int tray_debug_transform_table(TrayDeviceScene* s, uint32_t n, uint32_t* n_differ);

/* ---- one frame on several GPUs of this process ------------------------------------------------------
 * The reference's distributed mode hands every worker a slice of the block queue and sums the returned RGBW blocks on the
 * master (src/exec/distrib/master.rs:91-93,124-163; film::Image::add_blocks, src/film/image.rs:36-50). Here the workers are
 * the GPUs of one node: tray_multi_create deep-copies the scene to each listed device and creates one RCCL communicator per
 * device (ncclCommInitAll); the calls leave the calling thread's current HIP device as they found it; tray_render_frame_multi renders shard d of n_dev on device d (tray_render_shard_device, 16-tile
 * chunks round-robin, one host thread and one stream per device), sums the per-device films onto the first device with ONE
 * ncclReduce(sum) over xGMI and adds the result into rgbw_host (width*height*4 f32, get_renderf32 layout). A Rust
 * exec::Hip that owns a whole node calls these three instead of spawning worker processes. RCCL is loaded with dlopen
 * (librccl.so) when the first TrayMultiScene is created: a build or a box without it still serves the single-GPU calls. */
typedef struct TrayMultiScene TrayMultiScene;
int tray_multi_create(const TrayFlatScene* f, int n_dev, const int* dev_ids, TrayMultiScene** out);
int tray_render_frame_multi(TrayMultiScene* m, uint32_t spp, uint64_t seed, float* rgbw_host);
/* How tray_render_frame_multi splits a frame. TRAY_PARTITION_TILES (the default): device d renders shard d of the tiles (above).
 * TRAY_PARTITION_SAMPLES: every device renders every tile, device d the samples tray_multi_shard_samples gives it
 * (tray_render_samples_device) -- the same work per device by construction, where the reference deals blocks (exec/distrib/master.rs:91-93);
 * the films are summed by the same one ncclReduce (film/image.rs:21-50). A device whose range is empty (n_dev > spp) launches nothing and
 * joins the reduce. The render returns TRAY_E_UNSUPPORTED under TRAY_PARTITION_SAMPLES unless every device uses LowDiscrepancy (sampler/ld.rs).
 * TRAY_E_INVALID for an unknown partition. */
enum { TRAY_PARTITION_TILES = 0, TRAY_PARTITION_SAMPLES = 1 };
int tray_multi_set_partition(TrayMultiScene* m, int partition);          /* default TILES: today's behaviour */
/* host enumeration of device d's range under TRAY_PARTITION_SAMPLES: [floor(d*spp/n), floor((d+1)*spp/n)); TRAY_E_INVALID unless spp is a
 * power of two and d < n_dev */
int tray_multi_shard_samples(uint32_t spp, uint32_t d, uint32_t n_dev, uint32_t* begin, uint32_t* end);
/* tray_scene_set_sampler on every device of m */
int tray_multi_set_sampler(TrayMultiScene* m, uint32_t kind, uint32_t min_spp, uint32_t max_spp);
/* tray_scene_set_wavefront on every device of m */
int tray_multi_set_wavefront(TrayMultiScene* m, uint32_t pool_slots, uint32_t views, uint32_t slices);
/* tray_scene_set_transform_table on every device of m */
int tray_multi_set_transform_table(TrayMultiScene* m, int mode);
/* tray_scene_update_frame on every device of m; the communicators, films and streams are kept (scene.rs:152-176 per worker) */
int tray_multi_update_frame(TrayMultiScene* m, const TrayFlatScene* f);
/* per-device timings of the last tray_render_frame_multi (n_dev entries) and the duration of the reduce (ms) */
int tray_multi_timing(TrayMultiScene* m, TrayKernelTiming* per_device, float* reduce_ms);
void tray_multi_destroy(TrayMultiScene* m);

/* ---- parity / debug entry points (same device code as the renderer, one thread per item) ---- */

typedef struct TrayRay { float o[3]; float d[3]; float min_t, max_t, time; } TrayRay;   /* ray.rs:9-22 */
typedef struct TrayHit {
    float t;
    uint32_t inst;      /* instance id or 0xffffffff on miss */
    uint32_t prim;      /* triangle slot (leaf order) for meshes, else 0 */
    float p[3], n[3], ng[3];
    float u, v;
    float dp_du[3], dp_dv[3];
} TrayHit;
/* Scene::intersect (scene.rs:148-150) for n host rays -> n host hits. */
int tray_debug_intersect(TrayDeviceScene* s, uint32_t n, const TrayRay* rays, TrayHit* hits);

/* Radiance of individual camera samples: for item i, pixel (px[i], py[i]), sample index si[i]:
 * out[i*8 + 0..2] = clamped rgb (multithreaded.rs:98-99), [3] = sample x, [4] = sample y,
 * [5] = number of path vertices, [6] = number of rays, [7] = 0. */
int tray_debug_sample_radiance(TrayDeviceScene* s, uint32_t n, const uint32_t* px, const uint32_t* py,
                               const uint32_t* si, uint32_t spp, uint64_t seed, float* out);

/* The first hit of individual camera samples (tray_render_first_hit_device's per-sample statement), items as above:
 * out[i*12 + 0..2] = sample x, y, time, [3..5] = albedo rgb, [6..8] = normal xyz, [9] = t, [10] = hit, [11] = 0. */
int tray_debug_first_hit(TrayDeviceScene* s, uint32_t n, const uint32_t* px, const uint32_t* py, const uint32_t* si, uint32_t spp,
                         uint64_t seed, float* out);

/* BSDF::eval / pdf / sample (src/bxdf/bsdf.rs:66-125) of material `material_id` on a canonical
 * frame (n = +z, dp_du = +x). For item i: wo = dirs[i*6..+3], wi = dirs[i*6+3..+6], u = u3[i*3..+3]
 * (two_d.0, two_d.1, one_d). out[i*12]: eval rgb(3), pdf(1), sample f rgb(3), sample wi(3),
 * sample pdf(1), sampled type bits(1, as float). flags: 0 = BxDFType::all(), 1 = non_specular(). */
int tray_debug_bsdf(TrayDeviceScene* s, uint32_t material_id, uint32_t flags, uint32_t n,
                    const float* dirs, const float* u3, float* out);

const char* tray_last_error(void);
const char* tray_version(void);

/* sizeof() of the structs above as this library was compiled, for bindings that restate the layouts (ctypes, repr(C)):
 * name is the struct name ("TrayInstance", ...); 0 for an unknown name. */
uint32_t tray_abi_sizeof(const char* name);

#ifdef __cplusplus
}
#endif
#endif /* TRAYHIP_H */
