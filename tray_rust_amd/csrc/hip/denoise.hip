// libtrayhip_denoise.so: the kernels of tray_denoise_device (denoise_kernels.h) and their launches (denoise.h).
//   hipcc -c denoise.hip -o denoise.o
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "denoise_kernels.h"
#include "denoise.h"

namespace tr_denoise {

void prepare(hipStream_t stream, const float* even, const float* odd, uint32_t width, uint32_t height, void* scratch) {
    const float4* const e4 = reinterpret_cast<const float4*>(even);
    const float4* const o4 = reinterpret_cast<const float4*>(odd);
    float4* const s4 = static_cast<float4*>(scratch);
    const uint32_t blocks = (uint32_t)(((uint64_t)width * height + DN_PREP_BLOCK - 1u) / DN_PREP_BLOCK);
    hipLaunchKernelGGL(k_dn_prepare<0>, dim3(blocks), dim3(DN_PREP_BLOCK), 0, stream, e4, o4, width, height, s4);
    hipLaunchKernelGGL(k_dn_prepare<1>, dim3(blocks), dim3(DN_PREP_BLOCK), 0, stream, e4, o4, width, height, s4);
}

void denoise(hipStream_t stream, const float* even, const float* odd, uint32_t width, uint32_t height, uint32_t radius, uint32_t patch, float k, float* out,
             void* scratch) {
    prepare(stream, even, odd, width, height, scratch);
    const float4* const s4 = static_cast<const float4*>(scratch);
    float4* const out4 = reinterpret_cast<float4*>(out);
    dn_with_patch(patch, [&](auto f) {
        hipLaunchKernelGGL(k_dn_filter<decltype(f)::value>, dim3(dn_tiles_x(width) * dn_tiles_y(height)), dim3(DN_BLOCK), 0, stream, s4, width, height, radius,
                           k, out4);
    });
}

}  // namespace tr_denoise
