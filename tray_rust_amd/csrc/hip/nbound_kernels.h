// The per-round kernels of the neighbour bound of the two noise-target calls (include/trayhip.h: tray_scene_set_noise_ratio): the map from tile
// coordinates to queue indices, the pull step that flags a tile whose neighbour gets more than max_ratio times its samples, and the ordered
// compaction of one level's tile list. Device code only; compiled into libtrayhip_nbound.so by nbound.hip, and by g++ into the host emulation
// (tests/emu/emu_nbound.cpp). None of it is a hot path: a 1080p frame has 32 400 tiles.
#pragma once
#include "block_compact.h"

namespace tr_nbound {

#define NB_BLOCK 256u            // k_nb_grid, k_nb_pull: one thread per queue entry
#define NB_COMPACT_BLOCK 1024u   // k_nb_compact_level: the one workgroup
#define NB_NO_TILE 0xffffffffu   // a cell of the map that holds no tile of the call's range

// map[y * grid_w + x] = i for every queue entry i = (x, y) of queue[0, n); the launch function fills the map with NB_NO_TILE before. A tile
// outside the grid (no queue holds one) is left out.
__global__ __launch_bounds__(NB_BLOCK) void k_nb_grid(const uint2* __restrict__ queue, uint32_t n, uint32_t grid_w, uint32_t grid_h,
                                                      uint32_t* __restrict__ map) {
    const uint32_t i = blockIdx.x * NB_BLOCK + threadIdx.x;
    if (i >= n) return;   // (no barrier in this kernel)
    const uint2 t = queue[i];
    if (t.x < grid_w && t.y < grid_h) map[(size_t)t.y * grid_w + t.x] = i;
}

// One step of rule (b): queue entry i, with n_t = samples[i] < max_spp and its flag not set, sets its flag if one of the up to eight tiles around
// it in the map has n_u' > max_ratio * n_t, where n_u' = 2 n_u if u's flag is set and n_u otherwise. Flags are only ever set, and a flag is set
// only where the rule's least fixed point has it set, whatever mix of old and new flags of its neighbours a thread sees: launched as often as
// the longest chain of pulls is long (a pulled tile has fewer samples than the tile that pulled it: levels - 1), the flags are the fixed point.
// `active` is read and written by different threads of one launch, so it is not __restrict__; plain loads and stores, no atomics.
__global__ __launch_bounds__(NB_BLOCK) void k_nb_pull(const uint2* __restrict__ queue, uint32_t n, const uint32_t* __restrict__ map, uint32_t grid_w,
                                                      uint32_t grid_h, const uint32_t* __restrict__ samples, uint32_t* active, uint32_t max_ratio,
                                                      uint32_t max_spp) {
    const uint32_t i = blockIdx.x * NB_BLOCK + threadIdx.x;
    if (i >= n) return;   // (no barrier in this kernel)
    const uint32_t n_t = samples[i];
    if (active[i] != 0u || n_t >= max_spp) return;
    const uint2 t = queue[i];
    if (t.x >= grid_w || t.y >= grid_h) return;
    const uint64_t bound = (uint64_t)max_ratio * n_t;
    bool pulled = false;
    for (int dy = -1; dy <= 1; ++dy)
        for (int dx = -1; dx <= 1; ++dx) {
            const int64_t x = (int64_t)t.x + dx, y = (int64_t)t.y + dy;
            if ((dx == 0 && dy == 0) || x < 0 || y < 0 || x >= (int64_t)grid_w || y >= (int64_t)grid_h) continue;
            const uint32_t u = map[(size_t)y * grid_w + (size_t)x];
            if (u >= n) continue;   // (NB_NO_TILE: the tile is outside the call's range)
            const uint64_t n_u = (uint64_t)samples[u] * (active[u] != 0u ? 2u : 1u);
            pulled = pulled || n_u > bound;
        }
    if (pulled) active[i] = 1u;
}

// One level's tile list: the tiles of queue[0, n) whose flag is set and whose samples[i] == n_level, in queue order, as k_noise_compact writes
// the list of all flagged tiles (coordinates to out_tiles, queue indices to out_q, their number to *count). One workgroup walks the queue in
// steps of NB_COMPACT_BLOCK entries (block_compact.h; the loop's bound is uniform and no thread leaves before the last barrier).
__global__ __launch_bounds__(NB_COMPACT_BLOCK) void k_nb_compact_level(const uint2* __restrict__ queue, const uint32_t* __restrict__ active,
                                                                       const uint32_t* __restrict__ samples, uint32_t n_level, uint32_t n,
                                                                       uint2* __restrict__ out_tiles, uint32_t* __restrict__ out_q,
                                                                       uint32_t* __restrict__ count) {
    __shared__ uint32_t s_wave[NB_COMPACT_BLOCK / 64u];
    uint32_t total = 0u;
    for (uint32_t i0 = 0u; i0 < n; i0 += NB_COMPACT_BLOCK) {
        const uint32_t i = i0 + threadIdx.x;
        const bool keep = i < n && active[i] != 0u && samples[i] == n_level;
        const uint32_t o = tr::block_compact_slot<NB_COMPACT_BLOCK>(keep, total, s_wave);   // (o < n: at most one entry per queue index)
        if (keep) {
            out_tiles[o] = queue[i];
            out_q[o] = i;
        }
    }
    if (threadIdx.x == 0u) *count = total;
}

}  // namespace tr_nbound
