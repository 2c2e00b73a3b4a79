// One step of an ordered compaction by one workgroup of BLOCK threads (k_noise_compact, k_guide_compact): a ballot per wave, the waves' counts
// through LDS. Device code only. It holds two barriers, so every thread of the workgroup must call it, under control flow that is uniform over
// the workgroup (a loop whose bound every thread shares).
#pragma once
#include <stdint.h>

namespace tr {

// keep: whether this thread has an entry in this step. Returns the thread's slot: total + the entries kept by the threads before it (of use
// where keep; the order of the threads is the order of the output), and advances total -- the entries written before this step, the same in
// every thread -- by the step's entries. s_wave: BLOCK / 64 words of LDS, the workgroup's own.
template <uint32_t BLOCK>
__device__ __forceinline__ uint32_t block_compact_slot(bool keep, uint32_t& total, uint32_t* s_wave) {
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const unsigned long long m = __ballot(keep);
    if (lane == 0u) s_wave[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    uint32_t before = 0u, sum = 0u;
    for (uint32_t k = 0u; k < BLOCK / 64u; ++k) {
        const uint32_t c = s_wave[k];
        before += k < wave ? c : 0u;
        sum += c;
    }
    const uint32_t slot = total + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
    total += sum;
    __syncthreads();   // (s_wave is rewritten by the next step)
    return slot;
}

}  // namespace tr
