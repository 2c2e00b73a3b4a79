// libtrayhip_noise.so: the per-round kernels of tray_render_noise_target_device (noise_kernels.h) and their launches (noise.h).
//   hipcc -c noise.hip -o noise.o
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "noise_kernels.h"
#include "noise.h"

namespace tr_noise {

void error(hipStream_t stream, const float* even, const float* odd, uint32_t width, uint32_t height, const uint2* tiles, const uint32_t* qidx,
           uint32_t n_active, uint32_t n_taken, uint32_t max_spp, float threshold, float* err, uint32_t* active, uint32_t* samples) {
    const uint32_t per_block = NT_ERR_BLOCK / 64u;
    hipLaunchKernelGGL(k_noise_error, dim3((n_active + per_block - 1u) / per_block), dim3(NT_ERR_BLOCK), 0, stream, reinterpret_cast<const float4*>(even),
                       reinterpret_cast<const float4*>(odd), width, height, tiles, qidx, n_active, n_taken, max_spp, threshold, err, active, samples);
}

void compact(hipStream_t stream, const uint2* queue, const uint32_t* active, uint32_t n, uint2* out_tiles, uint32_t* out_q, uint32_t* count) {
    hipLaunchKernelGGL(k_noise_compact, dim3(1), dim3(NT_COMPACT_BLOCK), 0, stream, queue, active, n, out_tiles, out_q, count);
}

}  // namespace tr_noise
