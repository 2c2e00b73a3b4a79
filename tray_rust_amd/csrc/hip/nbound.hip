// libtrayhip_nbound.so: the kernels of the noise-target calls' neighbour bound (nbound_kernels.h) and their launches (nbound.h).
//   hipcc -c nbound.hip -o nbound.o
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "nbound_kernels.h"
#include "nbound.h"

namespace tr_nbound {

hipError_t grid(hipStream_t stream, const uint2* queue, uint32_t n, uint32_t grid_w, uint32_t grid_h, uint32_t* map) {
    if (const hipError_t e = hipMemsetAsync(map, 0xff, (size_t)grid_w * grid_h * sizeof(uint32_t), stream); e != hipSuccess) return e;
    hipLaunchKernelGGL(k_nb_grid, dim3((n + NB_BLOCK - 1u) / NB_BLOCK), dim3(NB_BLOCK), 0, stream, queue, n, grid_w, grid_h, map);
    return hipSuccess;
}

void pull(hipStream_t stream, const uint2* queue, uint32_t n, const uint32_t* map, uint32_t grid_w, uint32_t grid_h, const uint32_t* samples,
          uint32_t* active, uint32_t max_ratio, uint32_t max_spp) {
    hipLaunchKernelGGL(k_nb_pull, dim3((n + NB_BLOCK - 1u) / NB_BLOCK), dim3(NB_BLOCK), 0, stream, queue, n, map, grid_w, grid_h, samples, active,
                       max_ratio, max_spp);
}

void compact_level(hipStream_t stream, const uint2* queue, const uint32_t* active, const uint32_t* samples, uint32_t n_level, uint32_t n,
                   uint2* out_tiles, uint32_t* out_q, uint32_t* count) {
    hipLaunchKernelGGL(k_nb_compact_level, dim3(1), dim3(NB_COMPACT_BLOCK), 0, stream, queue, active, samples, n_level, n, out_tiles, out_q, count);
}

}  // namespace tr_nbound
