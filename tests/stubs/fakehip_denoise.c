/* The stand-in HIP runtime of tests/stubs/fakehip_noise.c (the tile-kernel log lines under FAKEHIP_TILE_KERNEL=1, one line per launch of a
 * kernel of libtrayhip_noise.so) with one line per launch of a kernel of libtrayhip_denoise.so as well ("denoise dev=.. grid=.. block=..
 * stream=.. kernel=<symbol>"): those launches are not tile kernels either, so their arguments are neither read nor written.
 * tests/test_denoise_stub.py. */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <string.h>
#define hipLaunchKernel fakehip_launch_kernel_base
#include "fakehip.c"
#undef hipLaunchKernel

hipError_t hipLaunchKernel(const void* f, dim3 g, dim3 b, void** args, size_t sh, hipStream_t st) {
    Dl_info di;
    const int found = dladdr(f, &di) && di.dli_fname;
    if (found && strstr(di.dli_fname, "libtrayhip_denoise") != NULL) {
        logf_("denoise dev=%d grid=%u block=%u stream=%p kernel=%s", t_device, g.x, b.x, st, di.dli_sname ? di.dli_sname : "?");
        return 0;
    }
    if (found && strstr(di.dli_fname, "libtrayhip_noise") != NULL) {
        logf_("noise dev=%d grid=%u block=%u kernel=%s", t_device, g.x, b.x, di.dli_sname ? di.dli_sname : "?");
        return 0;
    }
    if (getenv("FAKEHIP_TILE_KERNEL")) {
        const int ranged = found && strstr(di.dli_fname, "libtrayhip_ranges") != NULL;
        logf_("range dev=%d begin=%u end=%u", t_device, ranged ? *(uint32_t*)args[11] : 0u, ranged ? *(uint32_t*)args[12] : 0u);
    }
    return fakehip_launch_kernel_base(f, g, b, args, sh, st);
}
