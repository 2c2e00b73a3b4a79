// Host emulation of the kernels of tray_denoise_device (tray_rust_amd/csrc/hip/denoise_kernels.h): k_dn_prepare and k_dn_filter, compiled by g++
// behind hip_emu.h and run as SIMT fibers, so that the LDS staging, the per-offset barriers and the separable patch sums execute as the
// device executes them. Built by tests/test_denoise_emu.py; the other denoiser emulations include this file for EmuOps (emu_denoise_ops.h).
#include "emu_denoise_ops.h"

extern "C" {

uint64_t emu_denoise_scratch_bytes(uint32_t width, uint32_t height) { return dn_scratch_bytes(width, height); }

// one tray_denoise_device call: the plan's schedule (three launches); scratch: emu_denoise_scratch_bytes(width, height) bytes
int emu_denoise(const float* even, const float* odd, uint32_t width, uint32_t height, uint32_t radius, uint32_t patch, float k, float* out, void* scratch) {
    const dn::Params p{radius, 0u, patch, k};
    if (emu_refused(emu_filter_args(width, height, p))) return -2;
    EmuOps ops(width, height);
    dn::denoise(ops, dn::Frame{even, odd, nullptr, nullptr, nullptr}, p, out, scratch);
    return ops.rc;
}

}  // extern "C"
