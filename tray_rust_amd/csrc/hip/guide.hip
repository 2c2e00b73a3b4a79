// libtrayhip_guide.so: the kernels of tray_denoise_halves_device and of the filtered stopping rule (guide_kernels.h) and their launches (guide.h).
//   hipcc -c guide.hip -o guide.o
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "guide_kernels.h"
#include "guide.h"

namespace tr_guide {

static_assert(kBlockW == DN_TW && kBlockH == DN_TH, "guide.h states k_dn_filter's tile");
uint32_t blocks_x(uint32_t width) { return tr_denoise::dn_tiles_x(width); }
uint32_t blocks_y(uint32_t height) { return tr_denoise::dn_tiles_y(height); }

uint32_t halves(hipStream_t stream, const void* scratch, uint32_t width, uint32_t height, uint32_t radius, uint32_t patch, float k, const uint32_t* blocks,
                uint32_t n_blocks, float* fa, float* fb) {
    const uint32_t grid = blocks ? n_blocks : blocks_x(width) * blocks_y(height);
    if (grid == 0u) return 0u;
    const float4* const s4 = static_cast<const float4*>(scratch);
    float4* const a4 = reinterpret_cast<float4*>(fa);
    float4* const b4 = reinterpret_cast<float4*>(fb);
    dn_with_patch(patch, [&](auto f) {
        hipLaunchKernelGGL(k_dn_filter_halves<decltype(f)::value>, dim3(grid), dim3(DN_BLOCK), 0, stream, s4, width, height, radius, k, blocks, a4, b4);
    });
    return 1u;
}

void mark(hipStream_t stream, const uint2* queue, const uint32_t* active, uint32_t n, uint32_t width, uint32_t height, uint32_t* flags) {
    hipLaunchKernelGGL(k_guide_mark, dim3((n + GD_MARK_BLOCK - 1u) / GD_MARK_BLOCK), dim3(GD_MARK_BLOCK), 0, stream, queue, active, n, blocks_x(width),
                       blocks_y(height), flags);
}

void compact(hipStream_t stream, const uint32_t* flags, uint32_t width, uint32_t height, uint32_t* list, uint32_t* count) {
    hipLaunchKernelGGL(k_guide_compact, dim3(1), dim3(GD_COMPACT_BLOCK), 0, stream, flags, blocks_x(width) * blocks_y(height), list, count);
}

}  // namespace tr_guide
