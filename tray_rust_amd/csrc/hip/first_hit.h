// The first-hit launches (tray_render_first_hit_device, tray_debug_first_hit, tray_denoise_demodulated_device): k_first_hit_tiles,
// k_debug_first_hit, k_fh_demodulate and k_fh_remodulate (first_hit_kernels.h) live in libtrayhip_firsthit.so, compiled from first_hit.hip;
// device_api.hip launches them through these functions, so that libtrayhip.so's own code objects stay what they were.
#pragma once

namespace tr_firsthit {
// launches a demodulated call adds to its filter's: k_fh_demodulate before, k_fh_remodulate after
constexpr uint32_t kDemodLaunches = 2u;
// bytes of E' and O' behind the filter's scratch
inline uint64_t demod_bytes(uint32_t width, uint32_t height) { return (uint64_t)width * height * 32u; }
// one k_first_hit_tiles<anim> launch: a workgroup per tile of tiles[0 .. tile_count); anim = 0 (static), 2 (moving: the spline stacks are
// evaluated at every use, as the debug kernels do) or 3 (an AnimatedMesh)
void tiles(int anim, hipStream_t stream, size_t lds, const tr::DevScene& dev, const uint2* tiles, uint32_t tile_count, uint32_t spp, uint32_t kf,
           uint32_t smp_begin, uint32_t smp_end, float* albedo, float* normal, float* depth);
// one k_debug_first_hit<anim> launch over n items on the null stream
void debug(int anim, size_t lds, const tr::DevScene& dev, uint32_t n, const uint32_t* px, const uint32_t* py, const uint32_t* si, uint32_t spp,
           uint32_t kf, float* out);
// E' = (E.rgb / s, E.w), O' likewise, s from the albedo film
void demodulate(hipStream_t stream, const float* even, const float* odd, const float* albedo, uint32_t width, uint32_t height, float* even_out,
                float* odd_out);
// out = (out.rgb * s, 1)
void remodulate(hipStream_t stream, const float* albedo, uint32_t width, uint32_t height, float* out);
}  // namespace tr_firsthit
