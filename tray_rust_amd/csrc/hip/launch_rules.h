// The launch rules of the device-side C ABI (device_api.hip): what a launch renders and how its work is cut, as functions of plain integers -- no HIP
// call, no device scene. device_api.hip applies them to a TrayDeviceScene; the host emulation (tests/emu) compiles this header under g++ and applies the
// same functions to its own launches, so it tests the library's policy and keeps no copy of it. The measurements next to a rule are why its numbers are
// what they are. Environment overrides that belong to a rule are read here.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cstdlib>

#include "../../../include/trayhip.h"

#ifndef WF_MAX_SLICES
#define WF_MAX_SLICES 16u  // work items a tile's samples are cut into at most (k_wf_advance): the pool may hold that many chunks per tile
#endif

namespace tr_rules {

inline uint32_t round_spp(uint32_t spp) {   // ld.rs:22-25 (usize::next_power_of_two; 0 -> 1)
    uint32_t p = 1;
    while (p < spp && p < 0x80000000u) p <<= 1;
    return p;
}

inline uint32_t adaptive_step(uint32_t min_spp, uint32_t max_spp) {   // adaptive.rs:36-48
    const uint32_t lo = round_spp(min_spp), hi = round_spp(max_spp);
    return round_spp(hi > lo ? (hi - lo) / 5u : 0u);
}

// key_frame on the host (same mixing as the device function)
inline uint32_t frame_key(uint64_t seed, uint32_t frame) {
    auto mix = [](uint32_t x) { x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16; return x; };
    uint32_t kf = mix((uint32_t)seed + 0x9E3779B9u);
    kf = mix(kf ^ (uint32_t)(seed >> 32));
    return mix(kf + frame);
}

// tiles [tile_start, tile_start + tile_count) of a queue of n_tiles; count 0 means the whole queue
inline void clamp_tile_range(uint32_t n_tiles, uint32_t& tile_start, uint32_t& tile_count) {
    if (tile_count == 0) { tile_start = 0; tile_count = n_tiles; }          // BlockQueue::new ignores `start` when count == 0 (block_queue.rs:39-41), like tray_block_queue
    if (tile_start > n_tiles) tile_start = n_tiles;                         // skip(start).take(count)
    if (tile_count > n_tiles - tile_start) tile_count = n_tiles - tile_start;
}

// A sample range [smp_begin, smp_end) of the spp-sample frame; 0 / 0 = all of it. The whole frame as a range is the whole-frame launch.
inline void whole_frame_range(uint32_t spp, uint32_t smp_begin, uint32_t& smp_end) { if (smp_begin == 0u && smp_end == spp) smp_end = 0u; }
// samples per pixel a launch over the range renders
inline uint32_t range_samples(uint32_t spp, uint32_t smp_begin, uint32_t smp_end) { return smp_end ? smp_end - smp_begin : spp; }

// Work-item mapping of a launch: item w -> queue entry first + (w / chunk) * chunk_stride * chunk + (w % chunk)
struct TileWork { uint32_t first, work, chunk, chunk_stride; };
inline TileWork whole_queue(uint32_t tile_count) { return {0u, tile_count, tile_count ? tile_count : 1u, 1u}; }
// a shard's share: chunks c = shard, shard + n_shards, ... of chunk_tiles tiles each; the last chunk may be short (work 0: none of the chunks is this shard's)
inline TileWork shard_work(uint32_t n_tiles, uint32_t shard, uint32_t n_shards, uint32_t chunk_tiles) {
    const uint32_t n_chunks = (n_tiles + chunk_tiles - 1) / chunk_tiles;
    const uint32_t my_chunks = shard < n_chunks ? (n_chunks - shard + n_shards - 1) / n_shards : 0;
    if (my_chunks == 0) return {0u, 0u, 1u, 1u};
    const uint32_t last_chunk = shard + (my_chunks - 1) * n_shards;
    uint32_t tail = n_tiles - last_chunk * chunk_tiles;   // tiles in my last chunk
    if (tail > chunk_tiles) tail = chunk_tiles;
    return {shard * chunk_tiles, (my_chunks - 1) * chunk_tiles + tail, chunk_tiles, n_shards};
}

// Items per tile (k_path_tiles: progressive slices, level-major: the launch ends with its smallest items). A slice costs its own film resolve and
// flush and keeps >= 64 samples per pixel (>= 256 in a launch with many tiles per workgroup). Measured (profiles/r06_tile_slices_progressive_ab.txt, items per tile 1 / 2 / 3 / 4 / 5): the whole
// dragon frame 718.5 / 740.6 / 750.3 / 752.7 / 755.1 Msamples/s (tiles that show the mesh cost several times a wall tile: with whole tiles the last
// round of the 768 workgroups is one such tile), the whole cornell_box frame 1160.9 / 1163.5 / 1163.6 / 1159.9 / 1154.3; a GPU's eighth of the
// frame (4050 tiles, slowest of the eight shards against an eighth of the whole frame): dragon 0.449 / 0.632 / 0.784 / 0.862 / 0.872,
// cornell_box 0.895 / 0.942 / 0.960 / 0.971 / 0.975. So: three items per tile for a launch with many tiles per workgroup, up to five for a small one.
// TRAYHIP_TILE_SLICES=<items per tile> overrides. A sample range is cut by the same rules over its n_smp samples (k_path_tiles: any n_smp >= 1).
inline uint32_t tile_levels(uint32_t tile_count, uint32_t blocks, uint32_t n_smp) {
    uint32_t levels = 1u;
    {
        // (a launch with many tiles per workgroup keeps >= 256 samples per slice: at 256 spp three items per tile cost cornell_box 2.8 %, 1114 against 1146
        // Msamples/s, profiles/r06_c2_kept_gate_distance_ab.txt -- the resolves outweigh a tail that is 1 / 42 of the launch there)
        const bool small = tile_count < 12u * blocks;
        const uint32_t most = small ? 5u : 3u, least = small ? 64u : 256u;
        while (levels < most && (n_smp >> levels) >= least) ++levels;   // (the last two slices are spp >> (levels - 1) samples each)
    }
    if (const char* e = getenv("TRAYHIP_TILE_SLICES")) { levels = 1u; const uint32_t want = (uint32_t)std::max(1, atoi(e)); while (levels < want && (n_smp >> levels) >= 1u) ++levels; }
    return levels;
}

// The wavefront schedule: tiles are cut into 2^slice_shift slices of their n samples while the pool has at least as many chunks as the launch then has
// work items (k_wf_advance; a slice costs its own film resolve: at 8 M slots and 32 400 tiles halving them measured 124 against 132 Msamples/s); a
// slice keeps at least 16 samples per pixel and is never empty: 2^slice_shift <= n. req_slices (tray_scene_set_wavefront; 0 = this rule) and
// TRAYHIP_WF_SLICES override: 1, 2, 4, ...
inline uint32_t wf_slice_shift(uint32_t tile_count, uint32_t pool_chunks, uint32_t n, uint32_t req_slices) {
    uint32_t slice_shift = 0u;
    while ((1u << (slice_shift + 1u)) <= WF_MAX_SLICES && ((uint64_t)tile_count << (slice_shift + 1u)) <= pool_chunks && (n >> (slice_shift + 1u)) >= 16u) ++slice_shift;   // (cut while the items still fit the chunks: one item per chunk is the optimum)
    if (req_slices) { slice_shift = 0u; while ((2u << slice_shift) <= req_slices && (2u << slice_shift) <= WF_MAX_SLICES && (n >> (slice_shift + 1u)) >= 1u) ++slice_shift; }
    if (const char* e = getenv("TRAYHIP_WF_SLICES")) { slice_shift = 0u; while ((2u << slice_shift) <= (uint32_t)std::max(1, atoi(e)) && (2u << slice_shift) <= WF_MAX_SLICES && (n >> (slice_shift + 1u)) >= 1u) ++slice_shift; }
    return slice_shift;
}

// The sampler's plan (Pass: kernels.hip's SamplerPass with kind and the scene's min_spp / max_spp set): min_spp, max_spp, step and lum_cap of the
// launch; returns its rounds of k_sampler_pass.
template <class Pass>
inline uint32_t sampler_plan(Pass& sp, uint32_t spp) {
    uint32_t rounds = 1;
    if (sp.kind == TRAY_SAMPLER_LOW_DISCREPANCY) {   // (scenes with an AnimatedMesh: LowDiscrepancy::get_samples hands out all spp samples of a pixel at once, ld.rs:33-52)
        sp.min_spp = sp.max_spp = spp; sp.step = 1u; sp.lum_cap = 0u;
    } else if (sp.kind == TRAY_SAMPLER_ADAPTIVE) {
        sp.step = adaptive_step(sp.min_spp, sp.max_spp);
        while (sp.min_spp + (rounds - 1u) * sp.step < sp.max_spp) ++rounds;     // get_samples until samples_taken >= max_spp (adaptive.rs:136)
        sp.lum_cap = sp.min_spp + (rounds - 1u) * sp.step;
    } else { sp.min_spp = sp.max_spp = 1u; sp.step = 1u; sp.lum_cap = 0u; }
    return rounds;
}
// ... and the fields of round j; range_count: the samples of a LowDiscrepancy launch over a sample range (its samples of the spp-sample frame), 0 = the whole frame
template <class Pass>
inline void sampler_round(Pass& sp, uint32_t j, uint32_t range_count) {
    sp.pass = j;
    sp.count = sp.kind == TRAY_SAMPLER_ADAPTIVE ? (j == 0u ? sp.min_spp : sp.step) : sp.min_spp;   // (Uniform: 1, LowDiscrepancy: spp)
    if (sp.kind == TRAY_SAMPLER_LOW_DISCREPANCY && range_count) sp.count = range_count;
    sp.taken = sp.kind == TRAY_SAMPLER_ADAPTIVE ? sp.min_spp + j * sp.step : 0u;
    sp.before = j == 0u ? 0u : sp.min_spp + (j - 1u) * sp.step;
}
// (k_sampler_pass: a workgroup owns a group of consecutive tiles -- enough of them for ~4096 (pixel, sample) pairs of the round, group_max (16) at most: a
// 32 x 32 pixel square of the Z-order queue -- and hands the pairs to its lanes as their paths end)
inline uint32_t sampler_group(uint32_t count, int group_max) {
    const uint32_t per_tile = 64u * count;
    uint32_t group = std::max(1u, std::min<uint32_t>(group_max, 4096u / per_tile));
    if (const char* ge = getenv("TRAYHIP_SAMPLER_GROUP")) group = (uint32_t)std::max(1, std::min(group_max, atoi(ge)));   // (measurement; tests: ragged groups)
    return group;
}

}  // namespace tr_rules
