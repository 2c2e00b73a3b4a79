/* The stand-in HIP runtime of tests/stubs/fakehip_denoise.c (log lines of the tile kernels' sample ranges and of every launch of
 * libtrayhip_noise.so and libtrayhip_denoise.so) with one line per launch of a kernel of libtrayhip_guide.so as well ("guide dev=.. grid=..
 * block=.. stream=.. kernel=<symbol>"). The stand-in kernels do nothing, with one exception: a k_guide_compact launch (flags, n, list, count)
 * answers as if every flag were set -- list = 0 .. n - 1, *count = n --, so that the round that follows filters every block of the frame and
 * the launch shows in the log. tests/test_guide_stub.py. */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <string.h>
#define hipLaunchKernel fakehip_launch_kernel_base
#include "fakehip.c"
#undef hipLaunchKernel

hipError_t hipLaunchKernel(const void* f, dim3 g, dim3 b, void** args, size_t sh, hipStream_t st) {
    Dl_info di;
    const int found = dladdr(f, &di) && di.dli_fname;
    if (found && strstr(di.dli_fname, "libtrayhip_guide") != NULL) {
        const char* const sym = di.dli_sname ? di.dli_sname : "?";
        logf_("guide dev=%d grid=%u block=%u stream=%p kernel=%s", t_device, g.x, b.x, st, sym);
        if (strstr(sym, "k_guide_compact") != NULL) {
            const uint32_t n = *(uint32_t*)args[1];
            uint32_t* const list = *(uint32_t**)args[2];
            for (uint32_t i = 0; i < n; ++i) list[i] = i;
            **(uint32_t**)args[3] = n;
        }
        return 0;
    }
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
