// Host emulation of the kernels of the filtered stopping rule (tray_rust_amd/csrc/hip/guide_kernels.h): k_dn_filter_halves, k_guide_mark and
// k_guide_compact, compiled by g++ behind hip_emu.h and run as SIMT fibers, so that the LDS staging, the barriers, the ballots and the
// block-wide scan execute as the device executes them. Built by tests/test_guide_emu.py. Includes emu_denoise.cpp for EmuOps, and emu_noise.cpp and
// noise_plan.h (through noise_plan_record.h, whose exports ship here too) for the two noise-target calls at the end.
#include "emu_denoise.cpp"
#include "emu_noise.cpp"
#include "../../tray_rust_amd/csrc/hip/guide_kernels.h"
#include "noise_plan_record.h"

#include <cstring>
#include <vector>

using namespace tr_guide;

struct GuideOps : EmuOps {
    using EmuOps::EmuOps;
    // one k_dn_filter_halves<patch> launch as guide.hip makes it: over the list, or over every block when blocks is null
    void halves(const void* records, uint32_t radius, uint32_t patch, float k, const uint32_t* blocks, uint32_t n_blocks, float* fa, float* fb) {
        const float4* const s4 = emu_f4(records);
        float4* const a4 = emu_f4(fa), * const b4 = emu_f4(fb);
        run_tiles(blocks ? n_blocks : dn_tiles_x(width) * dn_tiles_y(height), patch,
                  [&](auto f) { k_dn_filter_halves<decltype(f)::value>(s4, width, height, radius, k, blocks, a4, b4); });
    }
};

extern "C" {

// one tray_denoise_halves_device call: the plan's schedule (k_dn_prepare<0>, <1>, k_dn_filter_halves<patch>; nothing for an empty list); scratch: 48
// bytes per pixel
int emu_guide_halves(const float* even, const float* odd, uint32_t width, uint32_t height, uint32_t radius, uint32_t patch, float k, const uint32_t* blocks,
                     uint32_t n_blocks, float* fa, float* fb, void* scratch) {
    const dn::Params p{radius, 0u, patch, k};
    if (emu_refused(emu_filter_args(width, height, p))) return -2;
    GuideOps ops(width, height);
    dn::halves(ops, dn::Frame{even, odd, nullptr, nullptr, nullptr}, p, blocks, n_blocks, fa, fb, scratch);
    return ops.rc;
}

// one k_guide_mark launch as guide.hip makes it; queue_xy: n (x, y) pairs, active: n words or null; flags: one word per block of the frame
int emu_guide_mark(const uint32_t* queue_xy, const uint32_t* active, uint32_t n, uint32_t width, uint32_t height, uint32_t* flags) {
    if (n == 0u) return 0;   // (the library never launches over an empty queue)
    std::vector<uint2> queue(n);
    for (uint32_t i = 0; i < n; ++i) queue[i] = make_uint2(queue_xy[2 * i], queue_xy[2 * i + 1]);
    return hip_emu::launch_simt((n + GD_MARK_BLOCK - 1u) / GD_MARK_BLOCK, GD_MARK_BLOCK,
                                [&] { k_guide_mark(queue.data(), active, n, dn_tiles_x(width), dn_tiles_y(height), flags); });
}

// one k_guide_compact launch as guide.hip makes it
int emu_guide_compact(const uint32_t* flags, uint32_t width, uint32_t height, uint32_t* list, uint32_t* count) {
    return hip_emu::launch_simt(1u, GD_COMPACT_BLOCK, [&] { k_guide_compact(flags, dn_tiles_x(width) * dn_tiles_y(height), list, count); });
}

}  // extern "C"

// ---- the two noise-target calls: noise_plan.h's schedule over the emulated kernels. The launch groups are the exports above and emu_noise.cpp's (a
// tile list is n (x, y) pairs of words there and here); what renders is the test's stand-in.

static_assert(DN_TW == TRAY_DENOISE_BLOCK_W && DN_TH == TRAY_DENOISE_BLOCK_H, "the plan's blocks are k_dn_filter's tiles");

// render: samples [begin, end) of the n tiles of list_xy into film; after_read: the round's kernels are done and its counts read. Non-zero stops the call.
typedef int (*emu_render_fn)(const uint32_t* list_xy, uint32_t n, uint32_t begin, uint32_t end, float* film);
typedef int (*emu_after_read_fn)(const uint32_t* counts, uint32_t n_words);

struct NoiseEmuOps : GuideOps {
    emu_render_fn render_fn;
    emu_after_read_fn after_read;
    NoiseEmuOps(uint32_t w, uint32_t h, emu_render_fn r, emu_after_read_fn a) : GuideOps(w, h), render_fn(r), after_read(a) {}
    static const uint32_t* xy(const void* tiles) { return static_cast<const uint32_t*>(tiles); }
    template <class F> int step(F&& f) { if (rc == 0) rc = f(); return rc; }   // (nothing runs after the first failure)
    int render(const void* list, uint32_t n, uint32_t begin, uint32_t end, float* film, uint32_t* launches) {
        *launches += 1u;
        return step([&] { return render_fn(xy(list), n, begin, end, film); });
    }
    int block_list(const void* queue, const uint32_t* active, uint32_t n, uint32_t* flags, uint32_t* list, uint32_t* count) {
        std::memset(flags, 0, (size_t)tr_ntplan::frame_blocks(width, height) * sizeof(uint32_t));
        step([&] { return emu_guide_mark(xy(queue), active, n, width, height, flags); });
        return step([&] { return emu_guide_compact(flags, width, height, list, count); });
    }
    int halves(const float* even, const float* odd, void* records, uint32_t radius, uint32_t patch, float k, const uint32_t* blocks, uint32_t n_blocks, float* fa,
               float* fb) {
        prepare(even, odd, records);
        if (n_blocks) GuideOps::halves(records, radius, patch, k, blocks, n_blocks, fa, fb);   // (guide.hip launches nothing over an empty list)
        return rc;
    }
    void error(const float* fe, const float* fo, const void* list, const uint32_t* list_q, uint32_t n, uint32_t taken, uint32_t max_spp, float threshold,
               float* err, uint32_t* active, uint32_t* samples) {
        step([&] { return emu_noise_error(fe, fo, width, height, xy(list), list_q, n, taken, max_spp, threshold, err, active, samples); });
    }
    void compact(const void* queue, const uint32_t* active, uint32_t n, void* list, uint32_t* list_q, uint32_t* count) {
        step([&] { return emu_noise_compact(xy(queue), active, n, static_cast<uint32_t*>(list), list_q, count); });
    }
    int read(const uint32_t* counts, uint32_t n_words, uint32_t* host) {
        std::memcpy(host, counts, n_words * sizeof(uint32_t));
        return step([&] { return after_read ? after_read(counts, n_words) : 0; });
    }
    int final_filter(const float* even, const float* odd, uint32_t radius, uint32_t patch, float k, float* out, void* records) {
        denoise(even, odd, radius, patch, k, out, records);
        return rc;
    }
};

extern "C" {

// One tray_render_noise_target_device call (scratch null) or one tray_render_noise_target_filtered_device call over queue_xy[0, tile_count): the
// plan's rules for the parameters (-2), then its schedule. tiles: tile_layout(n_tiles) bytes; scratch: filtered_layout(width, height) bytes; out may
// be null. Returns 0, the plan's refusal, or the first non-zero code of a fiber or a callback; *launches: the plan's count at one launch per render.
int emu_noise_target(const uint32_t* queue_xy, uint32_t tile_count, uint32_t n_tiles, uint32_t width, uint32_t height, uint32_t min_spp, uint32_t max_spp,
                     float threshold, float* even, float* odd, void* tiles, uint32_t radius, uint32_t patch, float k, void* scratch, float* out,
                     emu_render_fn render, emu_after_read_fn after_read, uint32_t* launches) {
    namespace nt = tr_ntplan;
    const nt::Scene s{true, TRAY_SAMPLER_LOW_DISCREPANCY, false, width, height};
    if (emu_refused(nt::target_rules("", s, min_spp, max_spp, threshold, even, odd, tiles, tiles))) return -2;
    if (scratch && emu_refused(emu_filter_args(width, height, dn::Params{radius, 0u, patch, k}))) return -2;
    if (tile_count == 0u || tile_count > n_tiles) return -2;
    NoiseEmuOps ops(width, height, render, after_read);
    const nt::Target t{queue_xy, tile_count, min_spp, max_spp, threshold, even, odd, tiles, n_tiles};
    const nt::Filter f{radius, patch, k, scratch, out};
    *launches = 0u;
    return nt::run(ops, t, scratch ? &f : nullptr, launches).rc;
}

}  // extern "C"
