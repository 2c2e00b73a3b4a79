// Host emulation of the kernels of the noise-target calls' neighbour bound (tray_rust_amd/csrc/hip/nbound_kernels.h): k_nb_grid, k_nb_pull and
// k_nb_compact_level, compiled by g++ behind hip_emu.h and run as SIMT fibers, and the two calls with a bound: noise_plan.h's schedule over the
// emulated kernels, the bound's groups added to emu_guide.cpp's Ops. Built by tests/_nbound_ref.py.
#include "emu_guide.cpp"
#include "../../tray_rust_amd/csrc/hip/nbound_kernels.h"

namespace {
std::vector<uint2> nb_tiles(const uint32_t* xy, uint32_t n) {
    std::vector<uint2> t(n);
    for (uint32_t i = 0; i < n; ++i) t[i] = make_uint2(xy[2 * i], xy[2 * i + 1]);
    return t;
}
}  // namespace

extern "C" {

// one tr_nbound::grid call as nbound.hip makes it: the memset, then k_nb_grid
int emu_nb_grid(const uint32_t* queue_xy, uint32_t n, uint32_t grid_w, uint32_t grid_h, uint32_t* map) {
    std::memset(map, 0xff, (size_t)grid_w * grid_h * sizeof(uint32_t));
    const std::vector<uint2> queue = nb_tiles(queue_xy, n);
    return hip_emu::launch_simt((n + NB_BLOCK - 1u) / NB_BLOCK, NB_BLOCK, [&] { tr_nbound::k_nb_grid(queue.data(), n, grid_w, grid_h, map); });
}

// one k_nb_pull launch as nbound.hip makes it
int emu_nb_pull(const uint32_t* queue_xy, uint32_t n, const uint32_t* map, uint32_t grid_w, uint32_t grid_h, const uint32_t* samples, uint32_t* active,
                uint32_t max_ratio, uint32_t max_spp) {
    const std::vector<uint2> queue = nb_tiles(queue_xy, n);
    return hip_emu::launch_simt((n + NB_BLOCK - 1u) / NB_BLOCK, NB_BLOCK,
                                [&] { tr_nbound::k_nb_pull(queue.data(), n, map, grid_w, grid_h, samples, active, max_ratio, max_spp); });
}

// one k_nb_compact_level launch as nbound.hip makes it: the flagged entries of queue_xy[0, n) with samples == n_level into out_xy / out_q
int emu_nb_compact_level(const uint32_t* queue_xy, const uint32_t* active, const uint32_t* samples, uint32_t n_level, uint32_t n, uint32_t* out_xy,
                         uint32_t* out_q, uint32_t* count) {
    const std::vector<uint2> queue = nb_tiles(queue_xy, n);
    std::vector<uint2> out(n);
    for (uint32_t i = 0; i < n; ++i) out[i] = make_uint2(out_xy[2 * i], out_xy[2 * i + 1]);   // (what the kernel leaves alone stays)
    const int rc = hip_emu::launch_simt(1u, NB_COMPACT_BLOCK,
                                        [&] { tr_nbound::k_nb_compact_level(queue.data(), active, samples, n_level, n, out.data(), out_q, count); });
    for (uint32_t i = 0; i < n; ++i) { out_xy[2 * i] = out[i].x; out_xy[2 * i + 1] = out[i].y; }
    return rc;
}

}  // extern "C"

struct NBoundEmuOps : NoiseEmuOps {
    using NoiseEmuOps::NoiseEmuOps;
    int grid(const void* queue, uint32_t n, uint32_t* map) {
        return step([&] { return emu_nb_grid(xy(queue), n, tr_ntplan::grid_w(width), tr_ntplan::grid_h(height), map); });
    }
    void pull(const void* queue, uint32_t n, const uint32_t* map, const uint32_t* samples, uint32_t* active, uint32_t max_ratio, uint32_t max_spp) {
        step([&] { return emu_nb_pull(xy(queue), n, map, tr_ntplan::grid_w(width), tr_ntplan::grid_h(height), samples, active, max_ratio, max_spp); });
    }
    void compact_level(const void* queue, const uint32_t* active, const uint32_t* samples, uint32_t n_level, uint32_t n, void* list, uint32_t* list_q,
                       uint32_t* count) {
        step([&] { return emu_nb_compact_level(xy(queue), active, samples, n_level, n, static_cast<uint32_t*>(list), list_q, count); });
    }
};

extern "C" {

// (offset, bytes) of the four regions of bound_layout in the order of the struct, then the total: 9 words
void emu_nbound_layout(uint32_t n_tiles, uint32_t grid_w, uint32_t grid_h, uint32_t levels, uint64_t* out) {
    const tr_ntplan::BoundLayout l = tr_ntplan::bound_layout(n_tiles, grid_w, grid_h, levels);
    const tr_ntplan::Region r[] = {l.lists, l.lists_q, l.map, l.counts};
    for (uint32_t i = 0; i < 4u; ++i) { out[2u * i] = r[i].offset; out[2u * i + 1u] = r[i].bytes; }
    out[8] = l.total;
}
uint32_t emu_nbound_call_launches(int filtered, int with_out, uint32_t rounds, uint32_t groups, uint32_t levels, uint32_t per_render) {
    return tr_ntplan::bound_call_launches(filtered != 0, with_out != 0, rounds, groups, levels, per_render);
}

// emu_noise_target (emu_guide.cpp) with a neighbour bound: max_ratio 0 runs the schedule without one, through the same entry point as the
// library's; bound: bound_layout(n_tiles, grid_w(width), grid_h(height), levels_of(min_spp, max_spp)) bytes
int emu_nbound_target(const uint32_t* queue_xy, uint32_t tile_count, uint32_t n_tiles, uint32_t width, uint32_t height, uint32_t min_spp, uint32_t max_spp,
                      float threshold, float* even, float* odd, void* tiles, uint32_t radius, uint32_t patch, float k, void* scratch, float* out,
                      uint32_t max_ratio, void* bound, emu_render_fn render, emu_after_read_fn after_read, uint32_t* launches) {
    namespace nt = tr_ntplan;
    const nt::Scene s{true, TRAY_SAMPLER_LOW_DISCREPANCY, false, width, height};
    if (emu_refused(nt::target_rules("", s, min_spp, max_spp, threshold, even, odd, tiles, tiles))) return -2;
    if (scratch && emu_refused(emu_filter_args(width, height, dn::Params{radius, 0u, patch, k}))) return -2;
    if (tile_count == 0u || tile_count > n_tiles || (max_ratio && !bound)) return -2;
    NBoundEmuOps ops(width, height, render, after_read);
    const nt::Target t{queue_xy, tile_count, min_spp, max_spp, threshold, even, odd, tiles, n_tiles};
    const nt::Filter f{radius, patch, k, scratch, out};
    const nt::Bound b{max_ratio, nt::grid_w(width), nt::grid_h(height), bound};
    *launches = 0u;
    return nt::run(ops, t, scratch ? &f : nullptr, launches, max_ratio ? &b : nullptr).rc;
}

}  // extern "C"
