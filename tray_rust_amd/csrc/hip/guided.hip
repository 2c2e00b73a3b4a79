// libtrayhip_guided.so: the kernel of tray_denoise_guided_device (guided_kernels.h) and its launch (guided.h).
//   hipcc -c guided.hip -o guided.o
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "guided_kernels.h"
#include "guided.h"

namespace tr_guided {

void filter(hipStream_t stream, const void* guide_records, const void* value_records, uint32_t width, uint32_t height, uint32_t radius, uint32_t patch, float k,
            float* out) {
    const float4* const g4 = static_cast<const float4*>(guide_records);
    const float4* const v4 = static_cast<const float4*>(value_records);
    float4* const out4 = reinterpret_cast<float4*>(out);
    dn_with_patch(patch, [&](auto f) {
        hipLaunchKernelGGL(k_gdn_filter<decltype(f)::value>, dim3(dn_tiles_x(width) * dn_tiles_y(height)), dim3(DN_BLOCK), 0, stream, g4, v4, width, height,
                           radius, k, out4);
    });
}

}  // namespace tr_guided
