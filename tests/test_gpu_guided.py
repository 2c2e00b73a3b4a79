"""The guided filter and the two-pass call on the GPU (tray_denoise_guided_device, tray_denoise_two_pass_device, Hip.denoise_guided,
Hip.denoise(passes=2), Hip.render_denoised(passes=2)).

Every comparison is with the f64 numpy statement of the call computed on the host (tests/_guided_ref.py) under its bar: 4 x what the f32
statement differs from the f64 one on the same films, plus 1e-7. The generator films (invalid pixels of every kind, a guide whose invalid pixels
are others), the films as their own guide against tray_denoise_device's bits, the two-pass call against its two parts' bits, the host
emulation's bits as a finding, films rendered by the tile kernel, where two passes must beat one, and a 1920 x 1080 call checked on crops. Two
calls give the same bits, guard bytes around the output and the scratch buffer stay intact, and the films are not written. Nothing here reads
the reference."""
import ctypes as C

import numpy as np
import pytest

import tray_rust_amd as T
from tray_rust_amd import scenes
import _denoise_ref as D
import _guided_ref as G
from _denoise_ref import denoise_guarded, rgb, rmse
from _guided_ref import guided_guarded, two_pass_guarded
from _noise_ref import load

pytestmark = pytest.mark.gpu

RF = [(1, 0), (3, 1), (7, 3), (10, 3)]
SIZES = [(67, 45), (160, 96)]
bits = lambda x: np.ascontiguousarray(x).view(np.uint32)


def films_and_guide(w, h):
    return D.random_films(w, h, seed=11 * w + h), D.random_films(w, h, seed=11 * w + h + 1000)


@pytest.mark.parametrize("r,f", RF, ids=[f"r{r}f{f}" for r, f in RF])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_generator_films_match_the_f64_statement(built, w, h, r, f):
    (even, odd), (ga, gb) = films_and_guide(w, h)
    out = guided_guarded(even, odd, ga, gb, r, f, 1.0)
    G.assert_guided(out, even, odd, ga, gb, r, f, 1.0, f"gpu {w}x{h} r={r} f={f}")
    again = guided_guarded(even, odd, ga, gb, r, f, 1.0)
    assert (bits(out) == bits(again)).all(), "two calls differ"
    assert len(D.range_violations(out[..., :3], even, odd, r, where=G.sure_pixels(even, odd, ga, gb))) == 0
    via_python = T.Hip(0).denoise_guided(even, odd, ga, gb, r, f, 1.0)
    assert isinstance(via_python, np.ndarray) and (bits(via_python) == bits(out)).all()


@pytest.mark.parametrize("r,f", RF, ids=[f"r{r}f{f}" for r, f in RF])
def test_the_films_as_their_own_guide_give_tray_denoise_devices_bits(built, r, f):
    for w, h in SIZES:
        even, odd = D.random_films(w, h, seed=11 * w + h)
        want = denoise_guarded(even, odd, r, f, 0.45)
        for got in (guided_guarded(even, odd, None, None, r, f, 0.45, alias=True), guided_guarded(even, odd, even, odd, r, f, 0.45)):
            assert (bits(got) == bits(want)).all(), (w, h, int((bits(got) != bits(want)).sum()))


def halves_on_device(even, odd, r, f, k):
    """tray_denoise_halves_device over every block; returns (fa, fb) as numpy films"""
    import torch
    h, w = even.shape[:2]
    lib = T.lib()
    e, o = (torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in (even, odd))
    fa, fb = torch.empty_like(e), torch.empty_like(e)
    scr = torch.empty(int(lib.tray_denoise_scratch_bytes(w, h)), dtype=torch.uint8, device="cuda")
    T.check(lib.tray_init(0))
    T.check(lib.tray_denoise_halves_device(w, h, C.c_void_p(e.data_ptr()), C.c_void_p(o.data_ptr()), r, f, k, None, 0, C.c_void_p(fa.data_ptr()),
                                           C.c_void_p(fb.data_ptr()), C.c_void_p(scr.data_ptr()), None))
    torch.cuda.synchronize()
    return fa.cpu().numpy(), fb.cpu().numpy()


@pytest.mark.parametrize("r,f", RF, ids=[f"r{r}f{f}" for r, f in RF])
def test_two_passes_are_halves_followed_by_guided(built, r, f):
    for (w, h), second in zip(SIZES, [(7, 3, 0.7), G.DEFAULTS2]):
        even, odd = D.random_films(w, h, seed=11 * w + h)
        fa, fb = halves_on_device(even, odd, r, f, 0.45)
        want = guided_guarded(even, odd, fa, fb, *second)
        got = two_pass_guarded(even, odd, r, f, 0.45, *second)
        assert (bits(got) == bits(want)).all(), (w, h, int((bits(got) != bits(want)).sum()))
        assert (bits(two_pass_guarded(even, odd, r, f, 0.45, *second)) == bits(got)).all(), "two calls differ"
    G.assert_two_pass(got, even, odd, r, f, 0.45, *second, f"gpu two passes {w}x{h} r={r} f={f}")
    via_python = T.Hip(0).denoise(even, odd, r, f, 0.45, passes=2)
    assert isinstance(via_python, np.ndarray) and (bits(via_python) == bits(got)).all()


def test_emulation_and_gpu_bits(built):
    """a finding, not a requirement: with tr::ref_expf on both sides and IEEE division the host emulation is expected to give the GPU's bits"""
    (even, odd), (ga, gb) = films_and_guide(67, 45)
    emu = G.guided_lib()   # (builds the emulation when called, here only)
    for r, f in RF:
        for what, gpu, cpu in (("guided", guided_guarded(even, odd, ga, gb, r, f, 1.0), G.run_guided(emu, even, odd, ga, gb, r, f, 1.0)),
                               ("two passes", two_pass_guarded(even, odd, r, f, 0.45, *G.DEFAULTS2), G.run_two_pass(emu, even, odd, r, f, 0.45, *G.DEFAULTS2))):
            n = int((bits(gpu) != bits(cpu)).sum())
            print(f"{what} r={r} f={f}: {n} of {gpu.size} words differ between the host emulation and the GPU (max abs {np.abs(gpu - cpu).max():.3e})")
            assert np.abs(gpu - cpu).max() <= 1e-5


def range_films(hip, scene, spp):
    """the films of [0, spp / 2) and [spp / 2, spp) of frame 0, rendered separately"""
    import torch
    fl = scene.flatten(0).contents.film
    w, h = fl.width, fl.height
    films = []
    for rng in ((0, spp // 2), (spp // 2, spp)):
        film = torch.zeros(w * h * 4, dtype=torch.float32, device="cuda:0")
        hip.render_samples_device(scene, 0, (0, 0), spp, rng, film.data_ptr())
        torch.cuda.synchronize()
        films.append(film.cpu().numpy().reshape(h, w, 4))
    return tuple(films)


W, H, SPP = 160, 96, 32


@pytest.mark.parametrize("name", ["cornell_box", "smallpt"])
def test_rendered_films(name, tmp_path):
    scene, rt, _, fi = load(getattr(scenes, name)(W, H, SPP), tmp_path)
    hip = T.Hip(0, seed=7)
    even, odd = range_films(hip, scene, SPP)
    r, f, k = 7, 3, 0.45
    one = hip.denoise(even, odd, r, f, k)
    two = hip.denoise(even, odd, passes=2)   # the defaults
    G.assert_two_pass(two, even, odd, r, f, k, *G.DEFAULTS2, f"{name} {W}x{H}x{SPP}, two passes")
    # render_denoised(passes=2) renders the same two ranges and shows denoise(passes=2) of them. A film is a sum of float atomics, so two renders
    # need not be the same bits: the bit comparison is made on the films render_denoised itself rendered, read at the filter's call, and those are
    # held against the separately rendered ones under tests/test_gpu_sample_ranges.py's bar for two renders of the same samples, 2e-5
    import torch
    seen, filt = [], hip._denoise_device

    def spy(e, o, *a):
        torch.cuda.synchronize()
        seen.append((e.cpu().numpy(), o.cpu().numpy(), a))
        return filt(e, o, *a)

    hip._denoise_device = spy
    hip.render_denoised(scene, rt, T.Config(str(tmp_path), "s.json", SPP, 1, fi), passes=2)
    hip._denoise_device = filt
    (e_, o_, args), = seen
    assert args == (r, f, k, G.DEFAULTS2), args
    shown = rt.get_renderf32().reshape(H, W, 4)
    assert (bits(shown) == bits(hip.denoise(e_, o_, passes=2))).all()
    for mine, separate in ((e_, even), (o_, odd)):
        assert np.abs(mine - separate).max() <= 2e-5 * max(1.0, float(np.abs(separate).max()))
    scene.release_device()
    ref = D.reference_image(scene, 4096, seed=1234)
    e0, e1, e2 = rmse(rgb(even + odd), ref), rmse(one[..., :3], ref), rmse(two[..., :3], ref)
    print(f"{name} {W}x{H} {SPP} spp: RMSE(noisy) = {e0:.5f}, RMSE(one pass) = {e1:.5f}, RMSE(two passes) = {e2:.5f}, ratio {e2 / e1:.3f}")
    assert e2 < e1 < e0
    # torch tensors in, a torch tensor out
    t = hip.denoise(*(torch.from_numpy(x).cuda() for x in (even, odd)), passes=2)
    assert isinstance(t, torch.Tensor) and t.is_cuda and (bits(t.cpu().numpy()) == bits(two)).all()


def test_full_size_call(tmp_path):
    """1920 x 1080, 16-spp cornell_box range films, two passes at the defaults: finite, weight 1, and three 96 x 96 crops (a corner, an edge, the
    centre) against the f64 statement of the sub-images; each is cut with radius + patch + max(radius2 + patch2, 1) + 2 surrounding pixels: the
    pilot's halo (with the 3 x 3 box of its variance) adds to the second pass's"""
    w, h, spp = 1920, 1080, 16
    r, f, k = 7, 3, 0.45
    r2, f2, k2 = G.DEFAULTS2
    scene, *_ = load(scenes.cornell_box(w, h, spp), tmp_path)
    even, odd = range_films(T.Hip(0, seed=3), scene, spp)
    got = T.Hip(0).denoise(even, odd, passes=2)
    assert np.isfinite(got).all() and (got[..., 3] == 1.0).all()
    m = r + f + max(r2 + f2, 1) + 2
    for what, (x0, y0) in [("corner", (0, 0)), ("edge", (w - 96, 500)), ("centre", (912, 492))]:
        xs0, ys0, xs1, ys1 = max(0, x0 - m), max(0, y0 - m), min(w, x0 + 96 + m), min(h, y0 + 96 + m)
        e, o = (np.ascontiguousarray(x[ys0:ys1, xs0:xs1]) for x in (even, odd))
        want, tol, err32, f32 = G.bar_of(lambda F: G.two_pass(e, o, r, f, k, r2, f2, k2, F))
        cut = (slice(y0 - ys0, y0 - ys0 + 96), slice(x0 - xs0, x0 - xs0 + 96))
        diff = np.abs(got[y0:y0 + 96, x0:x0 + 96, :3].astype(np.float64) - want[cut])
        err_cut = float(np.abs(f32.astype(np.float64) - want)[cut].max())
        print(f"1920x1080 {what} crop: kernels - f64 statement = {diff.max():.3e}, f32 statement - f64 statement = {err32:.3e} "
              f"({err_cut:.3e} inside the crop), bar {tol:.3e}")
        assert diff.max() <= tol, what
        assert diff.max() <= 4.0 * err_cut + 1e-7, f"{what}: {diff.max():.3e} > the crop's own bar {4.0 * err_cut + 1e-7:.3e}"
