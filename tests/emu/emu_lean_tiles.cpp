// TEST INFRASTRUCTURE ONLY: emu_kernels.cpp with the device source compiled as libtrayhip_tiles.so compiles it (csrc/hip/kernel_tiles.hip) -- the
// lean tile kernel behind the same entry points (tests/_lean_tiles_ref.py, tests/test_lean_tiles_emu.py).
#define TR_LEAN_TILES
#include "emu_kernels.cpp"
