// libtrayhip_firsthit.so: the first-hit kernels (first_hit_kernels.h) and their launches (first_hit.h), compiled as kernel_ranges.hip is -- the
// device functions of kernels.hip, and only the instantiations launched here.
//   hipcc -c first_hit.hip -o first_hit.o
#define TR_DEVICE_TU
#include "kernels.hip"
#include "first_hit_kernels.h"
#include "first_hit.h"

namespace tr_firsthit {

// past the default dynamic-LDS window the per-kernel limit is raised, as tray_scene_create raises it for libtrayhip.so's traversing kernels
template <class K>
static void allow_lds(K kernel, size_t lds) {
    if (lds > 32u * 1024u) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        (void)hipGetLastError();
    }
}
template <class K, class... A>
static void launch(K kernel, dim3 grid, size_t lds, hipStream_t stream, A... args) {
    allow_lds(kernel, lds);
    hipLaunchKernelGGL(kernel, grid, dim3(TR_BLOCK), lds, stream, args...);
}

void tiles(int anim, hipStream_t stream, size_t lds, const tr::DevScene& dev, const uint2* tiles, uint32_t tile_count, uint32_t spp, uint32_t kf,
           uint32_t smp_begin, uint32_t smp_end, float* albedo, float* normal, float* depth) {
    const dim3 grid(tile_count);
    if (anim == 3) launch(k_first_hit_tiles<3>, grid, lds, stream, dev, tiles, spp, kf, smp_begin, smp_end, albedo, normal, depth);
    else if (anim) launch(k_first_hit_tiles<2>, grid, lds, stream, dev, tiles, spp, kf, smp_begin, smp_end, albedo, normal, depth);
    else launch(k_first_hit_tiles<0>, grid, lds, stream, dev, tiles, spp, kf, smp_begin, smp_end, albedo, normal, depth);
}

void debug(int anim, size_t lds, const tr::DevScene& dev, uint32_t n, const uint32_t* px, const uint32_t* py, const uint32_t* si, uint32_t spp,
           uint32_t kf, float* out) {
    const dim3 grid((n + TR_BLOCK - 1) / TR_BLOCK);
    hipStream_t const null_stream = nullptr;
    if (anim == 3) launch(k_debug_first_hit<3>, grid, lds, null_stream, dev, n, px, py, si, spp, kf, out);
    else if (anim) launch(k_debug_first_hit<2>, grid, lds, null_stream, dev, n, px, py, si, spp, kf, out);
    else launch(k_debug_first_hit<0>, grid, lds, null_stream, dev, n, px, py, si, spp, kf, out);
}

static uint32_t pixels(uint32_t width, uint32_t height) { return width * height; }

void demodulate(hipStream_t stream, const float* even, const float* odd, const float* albedo, uint32_t width, uint32_t height, float* even_out,
                float* odd_out) {
    const uint32_t n = pixels(width, height);
    hipLaunchKernelGGL(k_fh_demodulate, dim3((n + TR_BLOCK - 1) / TR_BLOCK), dim3(TR_BLOCK), 0, stream, reinterpret_cast<const float4*>(even),
                       reinterpret_cast<const float4*>(odd), reinterpret_cast<const float4*>(albedo), n, reinterpret_cast<float4*>(even_out),
                       reinterpret_cast<float4*>(odd_out));
}

void remodulate(hipStream_t stream, const float* albedo, uint32_t width, uint32_t height, float* out) {
    const uint32_t n = pixels(width, height);
    hipLaunchKernelGGL(k_fh_remodulate, dim3((n + TR_BLOCK - 1) / TR_BLOCK), dim3(TR_BLOCK), 0, stream, reinterpret_cast<const float4*>(albedo), n,
                       reinterpret_cast<float4*>(out));
}

}  // namespace tr_firsthit
