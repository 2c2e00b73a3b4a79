"""The five device calls that run dn_filter_block (tray_denoise_device, tray_denoise_halves_device, tray_denoise_temporal_device,
tray_denoise_guided_device, tray_denoise_two_pass_device) on images of which every workgroup is partly or wholly outside: 9 x 5 (less than one
32 x 16 tile, and less than the radius: the whole halo is outside) and 33 x 17 (2 x 2 tiles; three of them hold one column, one row or one pixel).
That is where the read of the carried sums and the guards of the stores can go wrong, so every call runs between guard bytes.

Each output is held against the f64 numpy statement of its call under the bar of its own GPU file (4 x what the f32 statement differs from the
f64 one, plus 1e-7), and the three identities that one body gives by construction are asserted to the bit: one frame of the temporal filter,
the films as their own guide, and the mean of the halves each equal tray_denoise_device's output. The words that differ from the host
emulation are printed as a finding. Nothing here reads the reference."""
import functools

import numpy as np
import pytest

import _denoise_ref as D
import _emu_features as EF
import _guide_ref as GD
import _guided_ref as G
import _temporal_ref as TR
from _denoise_ref import denoise_guarded
from _guided_ref import guided_guarded, two_pass_guarded
from _temporal_ref import temporal_guarded
from test_gpu_guide import halves_guarded

pytestmark = pytest.mark.gpu

F32 = np.float32
SIZES = [(9, 5), (33, 17)]
RF = [(10, 3), (1, 0)]
K = 0.45
bits = lambda x: np.ascontiguousarray(x).view(np.uint32)


def finding(what, gpu, cpu):
    n = int((bits(gpu) != bits(cpu)).sum())
    print(f"{what}: {n} of {gpu.size} words differ between the host emulation and the GPU (max abs {np.abs(gpu - cpu).max():.3e})")
    assert np.abs(gpu - cpu).max() <= 1e-5


CASES = [(w, h, r, f) for w, h in SIZES for r, f in RF]
cases = pytest.mark.parametrize("w,h,r,f", CASES, ids=[f"{w}x{h}-r{r}f{f}" for w, h, r, f in CASES])


def films(w, h):
    """three frames of generator films, frames[0] the centre and the films of the single-frame calls"""
    return TR.random_frames(w, h, 3, seed=11 * w + h)


@functools.lru_cache(None)
def plain_of(w, h, r, f):
    """tray_denoise_device's output on films(w, h)[0]: computed once, compared by every test of a case and left as it is"""
    out = denoise_guarded(*films(w, h)[0], r, f, K)
    out.setflags(write=False)
    return out


@cases
def test_plain_and_halves(built, w, h, r, f):
    what = f"gpu {w}x{h} r={r} f={f}"
    even, odd = films(w, h)[0]
    plain = plain_of(w, h, r, f)
    D.assert_matches(plain, even, odd, r, f, K, what)
    finding(f"{what} plain", plain, EF.denoise(EF.denoise_lib(), even, odd, r, f, K))
    fa, fb = halves_guarded(even, odd, r, f, K)
    GD.assert_halves_match(fa, fb, even, odd, r, f, K, what)
    mean = ((fa[..., :3] + fb[..., :3]) * F32(0.5)).astype(F32)
    assert (bits(mean) == bits(plain[..., :3])).all(), "(fa + fb) * 0.5 is not tray_denoise_device's output to the bit"
    cpu = EF.guide_halves(EF.guide_lib(), even, odd, r, f, K)
    finding(f"{what} fa", fa, cpu[0])
    finding(f"{what} fb", fb, cpu[1])


@cases
def test_temporal(built, w, h, r, f):
    what = f"gpu {w}x{h} r={r} rt=1 f={f}"
    frames = films(w, h)
    plain = plain_of(w, h, r, f)
    one = temporal_guarded(frames[:1], r, 1, f, K)
    assert (bits(one) == bits(plain)).all(), ("one frame is not tray_denoise_device's output", int((bits(one) != bits(plain)).sum()))
    three = temporal_guarded(frames, r, 1, f, K)
    TR.assert_matches(three, frames, r, 1, f, K, f"{what} N=2")
    finding(f"{what} N=2", three, TR.run(TR.temporal_lib(), frames, r, 1, f, K))


@cases
def test_guided_and_two_passes(built, w, h, r, f):
    what = f"gpu {w}x{h} r={r} f={f}"
    even, odd = films(w, h)[0]
    ga, gb = D.random_films(w, h, seed=11 * w + h + 1000)
    plain = plain_of(w, h, r, f)
    for own in (guided_guarded(even, odd, None, None, r, f, K, alias=True), guided_guarded(even, odd, even, odd, r, f, K)):
        assert (bits(own) == bits(plain)).all(), ("the films as their own guide do not give tray_denoise_device's output", int((bits(own) != bits(plain)).sum()))
    guided = guided_guarded(even, odd, ga, gb, r, f, 1.0)
    G.assert_guided(guided, even, odd, ga, gb, r, f, 1.0, f"{what} guided")
    finding(f"{what} guided", guided, G.run_guided(G.guided_lib(), even, odd, ga, gb, r, f, 1.0))
    two = two_pass_guarded(even, odd, r, f, K, *G.DEFAULTS2)
    G.assert_two_pass(two, even, odd, r, f, K, *G.DEFAULTS2, f"{what} two passes")
    finding(f"{what} two passes", two, G.run_two_pass(G.guided_lib(), even, odd, r, f, K, *G.DEFAULTS2))
