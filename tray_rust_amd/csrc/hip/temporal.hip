// libtrayhip_temporal.so: the kernel of tray_denoise_temporal_device (temporal_kernels.h) and its launch (temporal.h).
//   hipcc -c temporal.hip -o temporal.o
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "temporal_kernels.h"
#include "temporal.h"

namespace tr_temporal {

void pass(hipStream_t stream, const void* centre_records, const void* frame_records, uint32_t width, uint32_t height, uint32_t radius, uint32_t patch, float k,
          void* sums, bool first, bool last, float* out) {
    const float4* const c4 = static_cast<const float4*>(centre_records);
    const float4* const f4 = static_cast<const float4*>(frame_records);
    float4* const acc4 = static_cast<float4*>(sums);
    float4* const out4 = reinterpret_cast<float4*>(out);
    dn_with_patch(patch, [&](auto f) {
        hipLaunchKernelGGL(k_tdn_pass<decltype(f)::value>, dim3(dn_tiles_x(width) * dn_tiles_y(height)), dim3(DN_BLOCK), 0, stream, c4, f4, width, height,
                           radius, k, acc4, first ? 1u : 0u, last ? 1u : 0u, out4);
    });
}

}  // namespace tr_temporal
