"""The one copy of the denoiser calls' scratch layouts and schedules (tray_rust_amd/csrc/hip/denoise_plan.h), which libtrayhip.so and the host emulation
both run: every call's regions are 16-byte aligned, pairwise disjoint and end at the plan's total; the total is the kernel header's *_scratch_bytes
(as the emulation libraries export them); the offsets per pixel are the ones the *_kernels.h comments document; and a recording Ops counts the
launches each schedule makes with N neighbours. The plan is reached through exports of the emulation library of the demodulated two-pass temporal
calls (tests/emu/emu_td2pass.cpp, denoise_plan_record.h). No GPU."""
import ctypes as C

import numpy as np
import pytest

import _emu_features as EF
import _guided_ref as G
import _td2pass_ref as X
import _tdemod_ref as TD
import _temporal_ref as TR
import _temporal2_ref as T2

SIZES = [(1, 1), (33, 17), (70, 40), (65535, 65535)]   # the last: the products need 64 bits
NEIGHBOURS = [0, 1, 2, 8]

# dn_record::Call of tests/emu/denoise_plan_record.h, in its order: (name; the documented offsets per pixel of the regions, then the total; which
# library's export holds the kernel header's total, and what the demodulated one-frame call adds behind it: E' and O'; launches with N neighbours)
FILM = 16   # bytes per pixel of an RGBW film
TEMPORAL = (0, 48, 96, 128)                             # centre, neighbour, sums (temporal_kernels.h)
TEMPORAL_GUIDED = (0, 48, 96, 144, 176)                 # centre_guide, guide, values, sums (t2pass_kernels.h)
TEMPORAL_TWO_PASS = (0, 48, 96, 128, 144, 160, 208, 256)   # centre, neighbour, sums, fa, fb, centre_guide, guide (t2pass_kernels.h)
CALLS = [
    ("denoise", (0, 48), (EF.denoise_lib, "emu_denoise_scratch_bytes", 0), lambda n: 3),
    ("halves", (0, 48), (EF.denoise_lib, "emu_denoise_scratch_bytes", 0), lambda n: 3),
    ("guided", (0, 48, 96), (G.guided_lib, "emu_guided_scratch_bytes", 0), lambda n: 5),                       # values, guide (guided_kernels.h)
    ("two_pass", (0, 48, 64, 80, 128), (G.guided_lib, "emu_two_pass_scratch_bytes", 0), lambda n: 6),          # values, fa, fb, guide
    ("demodulated", (0, 48, 64, 80), (EF.denoise_lib, "emu_denoise_scratch_bytes", 2 * FILM), lambda n: 5),    # the filter's, E', O'
    ("demodulated, two passes", (0, 128, 144, 160), (G.guided_lib, "emu_two_pass_scratch_bytes", 2 * FILM), lambda n: 8),
    ("temporal", TEMPORAL, (TR.temporal_lib, "emu_temporal_scratch_bytes", 0), lambda n: 3 * (n + 1)),
    ("temporal_demodulated", TEMPORAL, (TD.tdemod_lib, "emu_tdemod_scratch_bytes", 0), lambda n: 3 * (n + 1)),
    ("temporal_halves", TEMPORAL, (T2.temporal2_lib, "emu_temporal_halves_scratch_bytes", 0), lambda n: 3 * (n + 1)),
    ("temporal_guided", TEMPORAL_GUIDED, (T2.temporal2_lib, "emu_temporal_guided_scratch_bytes", 0), lambda n: 5 * (n + 1)),
    ("temporal_two_pass", TEMPORAL_TWO_PASS, (T2.temporal2_lib, "emu_temporal_two_pass_scratch_bytes", 0), lambda n: 9 * n + 6),
    ("temporal_demodulated_halves", TEMPORAL, (X.td2pass_lib, "emu_td2_halves_scratch_bytes", 0), lambda n: 3 * (n + 1)),
    ("temporal_demodulated_guided", TEMPORAL_GUIDED, (X.td2pass_lib, "emu_td2_guided_scratch_bytes", 0), lambda n: 5 * (n + 1)),
    ("temporal_demodulated_two_pass", TEMPORAL_TWO_PASS, (X.td2pass_lib, "emu_td2_two_pass_scratch_bytes", 0), lambda n: 9 * n + 6),
]
IDS = [c[0] for c in CALLS]


@pytest.fixture(scope="module")
def plan():
    return X.td2pass_lib()


def layout(plan, call, w, h):
    """([(offset, bytes)], total) of the plan's layout of call number `call`"""
    regions = np.zeros(2 * 8, np.uint64)
    total = C.c_uint64(0)
    n = plan.emu_denoise_plan_layout(call, w, h, regions.ctypes.data, 8, C.byref(total))
    assert 1 <= n <= 8
    return [(int(regions[2 * i]), int(regions[2 * i + 1])) for i in range(n)], int(total.value)


@pytest.mark.parametrize("call", range(len(CALLS)), ids=IDS)
def test_layout(plan, call):
    name, per_pixel, (lib, export, behind), _ = CALLS[call]
    for w, h in SIZES:
        px = w * h
        regions, total = layout(plan, call, w, h)
        assert [off for off, _ in regions] + [total] == [px * b for b in per_pixel], (name, w, h)   # the documented offsets
        assert all(off % 16 == 0 and size > 0 for off, size in regions), (name, w, h)
        ends = [off + size for off, size in regions]
        assert all(a <= off for a, (off, _) in zip(ends, regions[1:])), (name, w, h)   # in rising order: pairwise disjoint
        assert ends[-1] == total, (name, w, h)
        assert total == int(getattr(lib(), export)(w, h)) + px * behind, (name, w, h)   # the kernel header's


@pytest.mark.parametrize("call", range(len(CALLS)), ids=IDS)
def test_launches(plan, call):
    name, _, _, launches = CALLS[call]
    for n in NEIGHBOURS if name.startswith("temporal") else [0]:
        assert plan.emu_denoise_plan_launches(call, n) == launches(n), (name, n)
