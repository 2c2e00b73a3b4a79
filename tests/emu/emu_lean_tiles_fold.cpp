// TEST INFRASTRUCTURE ONLY: emu_kernels.cpp with the device source compiled as libtrayhip_foldmis.so compiles it (csrc/hip/kernel_fold.hip) -- the
// lean tile kernel WITH its re-timed item, TR_LEAN_FOLD_MIS_RAY (csrc/hip/dev_integrator.h) -- behind the same entry points
// (tests/test_lean_fold_emu.py). -DTR_LEAN_FOLD_MIN_LANES=<K> builds another threshold than the shipped one.
#define TR_LEAN_TILES
#define TR_LEAN_FOLD_MIS_RAY
// stage C rays k_path_tiles folded into the next step's stage A pass since the last call (kernels.hip counts them in the host emulation only)
unsigned long long tr_fold_rays = 0ull;
extern "C" unsigned long long emu_fold_rays(void) { const unsigned long long n = tr_fold_rays; tr_fold_rays = 0ull; return n; }
#include "emu_kernels.cpp"
extern "C" unsigned emu_fold_min_lanes(void) { return (unsigned)(TR_LEAN_FOLD_MIN_LANES); }
