// libtrayhip_tdemod.so: the kernels of tray_denoise_temporal_demodulated_device (tdemod_kernels.h) and their launches (tdemod.h).
//   hipcc -c tdemod.hip -o tdemod.o
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "tdemod_kernels.h"
#include "tdemod.h"

namespace tr_tdemod {

void prepare(hipStream_t stream, const float* even, const float* odd, const float* albedo, uint32_t width, uint32_t height, void* records) {
    const float4* const e4 = reinterpret_cast<const float4*>(even);
    const float4* const o4 = reinterpret_cast<const float4*>(odd);
    const float4* const a4 = reinterpret_cast<const float4*>(albedo);
    float4* const s4 = static_cast<float4*>(records);
    const uint32_t blocks = (uint32_t)(((uint64_t)width * height + DN_PREP_BLOCK - 1u) / DN_PREP_BLOCK);
    hipLaunchKernelGGL(k_tdm_prepare, dim3(blocks), dim3(DN_PREP_BLOCK), 0, stream, e4, o4, a4, width, height, s4);
    // (pass 1 reads the records only: the films' pointers are not dereferenced)
    hipLaunchKernelGGL(k_dn_prepare<1>, dim3(blocks), dim3(DN_PREP_BLOCK), 0, stream, e4, o4, width, height, s4);
}

void pass(hipStream_t stream, const void* centre_records, const void* frame_records, const float* albedo, uint32_t width, uint32_t height, uint32_t radius,
          uint32_t patch, float k, void* sums, bool first, bool last, float* out) {
    const float4* const c4 = static_cast<const float4*>(centre_records);
    const float4* const f4 = static_cast<const float4*>(frame_records);
    const float4* const a4 = reinterpret_cast<const float4*>(albedo);
    float4* const acc4 = static_cast<float4*>(sums);
    float4* const out4 = reinterpret_cast<float4*>(out);
    dn_with_patch(patch, [&](auto f) {
        hipLaunchKernelGGL(k_tdm_pass<decltype(f)::value>, dim3(dn_tiles_x(width) * dn_tiles_y(height)), dim3(DN_BLOCK), 0, stream, c4, f4, a4, width, height,
                           radius, k, acc4, first ? 1u : 0u, last ? 1u : 0u, out4);
    });
}

}  // namespace tr_tdemod
