// The per-round epilogue of tray_render_noise_target_device (include/trayhip.h): the two-buffer error of every active tile and the ordered
// compaction of the next round's tile list. Device code only; compiled into libtrayhip_noise.so by noise.hip, and by g++ into the host emulation
// (tests/emu/emu_noise.cpp).
#pragma once
#include "block_compact.h"

namespace tr_noise {

#define NT_ERR_BLOCK 256u       // k_noise_error: four waves, one tile each
#define NT_COMPACT_BLOCK 1024u  // k_noise_compact: the one workgroup

// The error of one pixel from its even film E and odd film O (include/trayhip.h): d / (1e-4 + sqrt(m)), +inf where a film has no weight.
// A NaN in either film gives NaN. The operations are the header's, in its order (tests compare with a numpy statement of them). The weight test
// selects at the end instead of returning early: every component is used on every path, so each film's pixel is one float4 load.
__device__ __forceinline__ float nt_pixel_error(float4 E, float4 O) {
    const float er = E.x / E.w, eg = E.y / E.w, eb = E.z / E.w;
    const float orr = O.x / O.w, og = O.y / O.w, ob = O.z / O.w;
    const float d = (fabsf(er - orr) + fabsf(eg - og) + fabsf(eb - ob)) * 0.5f;
    const float s = ((er + eg + eb) + (orr + og + ob)) * 0.5f;
    const float m = s > 0.0f ? s : 0.0f;
    const float err = d / (1e-4f + sqrtf(m));
    return (E.w <= 0.0f || O.w <= 0.0f) ? INFINITY : err;
}

// the larger of two errors; NaN if either is NaN (the tile then stays active: its error is not < threshold)
__device__ __forceinline__ float nt_max(float a, float b) { return (a > b || a != a) ? a : b; }

// One wave per tile of the active list, one lane per pixel: (x, y) = (lane & 7, lane >> 3) of the 8 x 8 tile, one float4 from each film. The
// tile's error is the maximum over its pixels inside the image, reduced across the wave with __shfl_xor. Lane 0 writes, by queue index
// (qidx[t], or t itself when qidx is null: round 0 renders the whole range), the error, the samples taken (n_taken) and whether the tile renders
// the next round: !(error < threshold) and n_taken < max_spp.
__global__ __launch_bounds__(NT_ERR_BLOCK) void k_noise_error(const float4* __restrict__ even, const float4* __restrict__ odd, uint32_t width,
                                                              uint32_t height, const uint2* __restrict__ tiles, const uint32_t* __restrict__ qidx,
                                                              uint32_t n_active, uint32_t n_taken, uint32_t max_spp, float threshold,
                                                              float* __restrict__ err, uint32_t* __restrict__ active, uint32_t* __restrict__ samples) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t t = blockIdx.x * (NT_ERR_BLOCK / 64u) + (threadIdx.x >> 6);
    if (t >= n_active) return;   // (whole waves: the shuffles below see all 64 lanes)
    const uint2 tile = tiles[t];
    const uint32_t px = tile.x * 8u + (lane & 7u), py = tile.y * 8u + (lane >> 3);
    float e = 0.0f;              // (pixels outside the image: every error is >= 0 or NaN)
    if (px < width && py < height) {
        const size_t p = (size_t)py * width + px;
        e = nt_pixel_error(even[p], odd[p]);
    }
    for (int k = 32; k >= 1; k >>= 1) e = nt_max(e, __shfl_xor(e, k));
    if (lane == 0u) {
        const uint32_t q = qidx ? qidx[t] : t;
        err[q] = e;
        samples[q] = n_taken;
        active[q] = (!(e < threshold) && n_taken < max_spp) ? 1u : 0u;
    }
}

// The next round's tile list: the tiles of queue[0, n) whose active flag is set, in queue order (so the tile kernel and the wavefront's chunks
// keep the Morton order, and the list is the same in every run), each as its coordinates (out_tiles) and its queue index (out_q); their number
// goes to *count. One workgroup walks the queue in steps of NT_COMPACT_BLOCK entries (block_compact.h; the loop's bound is uniform).
__global__ __launch_bounds__(NT_COMPACT_BLOCK) void k_noise_compact(const uint2* __restrict__ queue, const uint32_t* __restrict__ active, uint32_t n,
                                                                    uint2* __restrict__ out_tiles, uint32_t* __restrict__ out_q,
                                                                    uint32_t* __restrict__ count) {
    __shared__ uint32_t s_wave[NT_COMPACT_BLOCK / 64u];
    uint32_t total = 0u;
    for (uint32_t i0 = 0u; i0 < n; i0 += NT_COMPACT_BLOCK) {
        const uint32_t i = i0 + threadIdx.x;
        const bool keep = i < n && active[i] != 0u;
        const uint32_t o = tr::block_compact_slot<NT_COMPACT_BLOCK>(keep, total, s_wave);   // (o < n: at most one entry per queue index)
        if (keep) {
            out_tiles[o] = queue[i];
            out_q[o] = i;
        }
    }
    if (threadIdx.x == 0u) *count = total;
}

}  // namespace tr_noise
