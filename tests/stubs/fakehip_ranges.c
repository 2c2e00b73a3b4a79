/* The stand-in HIP runtime of tests/stubs/fakehip.c with one more log line per tile-kernel launch (FAKEHIP_TILE_KERNEL=1): the sample range
 * the kernel renders, written just before the launch's own line. The range instantiations live in libtrayhip_ranges.so (kernel_ranges.hip) and
 * take [smp_begin, smp_end) as their two trailing arguments (args[11], args[12]); a kernel of libtrayhip.so renders the whole frame: 0 / 0.
 * tests/test_sample_ranges_stub.py. */
#define _GNU_SOURCE
#include <dlfcn.h>
#include <string.h>
#define hipLaunchKernel fakehip_launch_kernel_base
#include "fakehip.c"
#undef hipLaunchKernel

hipError_t hipLaunchKernel(const void* f, dim3 g, dim3 b, void** args, size_t sh, hipStream_t st) {
    if (getenv("FAKEHIP_TILE_KERNEL")) {
        Dl_info di;
        const int ranged = dladdr(f, &di) && di.dli_fname && strstr(di.dli_fname, "libtrayhip_ranges") != NULL;
        logf_("range dev=%d begin=%u end=%u", t_device, ranged ? *(uint32_t*)args[11] : 0u, ranged ? *(uint32_t*)args[12] : 0u);
    }
    return fakehip_launch_kernel_base(f, g, b, args, sh, st);
}
