// libtrayhip_t2pass.so: the kernels of tray_denoise_temporal_halves_device / _guided_device / _two_pass_device (t2pass_kernels.h) and their
// launches (t2pass.h).
//   hipcc -c t2pass.hip -o t2pass.o
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "t2pass_kernels.h"
#include "t2pass.h"

namespace tr_t2pass {

void halves_pass(hipStream_t stream, const void* centre_records, const void* frame_records, uint32_t width, uint32_t height, uint32_t radius, uint32_t patch,
                 float k, void* sums, bool first, bool last, float* fa, float* fb) {
    const float4* const c4 = static_cast<const float4*>(centre_records);
    const float4* const f4 = static_cast<const float4*>(frame_records);
    float4* const acc4 = static_cast<float4*>(sums);
    float4* const fa4 = reinterpret_cast<float4*>(fa);
    float4* const fb4 = reinterpret_cast<float4*>(fb);
    dn_with_patch(patch, [&](auto f) {
        hipLaunchKernelGGL(k_t2p_halves_pass<decltype(f)::value>, dim3(dn_tiles_x(width) * dn_tiles_y(height)), dim3(DN_BLOCK), 0, stream, c4, f4, width,
                           height, radius, k, acc4, first ? 1u : 0u, last ? 1u : 0u, fa4, fb4);
    });
}

void guided_pass(hipStream_t stream, const void* centre_guide_records, const void* guide_records, const void* value_records, uint32_t width, uint32_t height,
                 uint32_t radius, uint32_t patch, float k, void* sums, bool first, bool last, float* out) {
    const float4* const c4 = static_cast<const float4*>(centre_guide_records);
    const float4* const g4 = static_cast<const float4*>(guide_records);
    const float4* const v4 = static_cast<const float4*>(value_records);
    float4* const acc4 = static_cast<float4*>(sums);
    float4* const out4 = reinterpret_cast<float4*>(out);
    dn_with_patch(patch, [&](auto f) {
        hipLaunchKernelGGL(k_t2p_guided_pass<decltype(f)::value>, dim3(dn_tiles_x(width) * dn_tiles_y(height)), dim3(DN_BLOCK), 0, stream, c4, g4, v4, width,
                           height, radius, k, acc4, first ? 1u : 0u, last ? 1u : 0u, out4);
    });
}

}  // namespace tr_t2pass
