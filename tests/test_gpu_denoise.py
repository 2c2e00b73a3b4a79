"""The dual-buffer NL-means denoiser on the GPU (tray_denoise_device, Hip.denoise, Hip.render_denoised).

Every comparison is with the f64 numpy statement of the filter computed on the host (tests/_denoise_ref.py) under its bar: 4 x what the f32
statement differs from the f64 one on the same films, plus 1e-7. The generator films (invalid pixels of every kind), films rendered by the tile
kernel and by the wavefront schedule, Hip.render_denoised against Hip.denoise of separately rendered films, and a 1920 x 1080 frame checked on
crops. Two calls give the same bits, and guard words around the output and the scratch buffer stay intact. Nothing here reads the reference."""
import ctypes as C

import numpy as np
import pytest

import tray_rust_amd as T
from tray_rust_amd import scenes
import _denoise_ref as D
from _denoise_ref import denoise_guarded, reference_image, rgb, rmse
from _noise_ref import load

pytestmark = pytest.mark.gpu

RF = [(1, 0), (3, 1), (7, 3), (10, 3)]


@pytest.mark.parametrize("r,f", RF, ids=[f"r{r}f{f}" for r, f in RF])
@pytest.mark.parametrize("w,h", [(67, 45), (160, 96)], ids=["67x45", "160x96"])
def test_generator_films_match_the_f64_statement(built, w, h, r, f):
    even, odd = D.random_films(w, h, seed=11 * w + h)
    out = denoise_guarded(even, odd, r, f, 0.45)
    D.assert_matches(out, even, odd, r, f, 0.45, f"gpu {w}x{h} r={r} f={f}")
    again = denoise_guarded(even, odd, r, f, 0.45)
    assert (out.view(np.uint32) == again.view(np.uint32)).all(), "two calls differ"
    assert len(D.range_violations(out[..., :3], even, odd, r)) == 0
    via_python = T.Hip(0).denoise(even, odd, r, f, 0.45)
    assert isinstance(via_python, np.ndarray) and (via_python.view(np.uint32) == out.view(np.uint32)).all()


def test_emulation_and_gpu_bits(built):
    """a finding, not a requirement: with tr::ref_expf on both sides and IEEE division the host emulation is expected to give the GPU's bits"""
    import _emu_features as EF   # (builds the emulation of the denoiser when called, here only)
    even, odd = D.random_films(67, 45, seed=5)
    emu = EF.denoise_lib()
    for r, f in RF:
        gpu = denoise_guarded(even, odd, r, f, 0.45)
        cpu = EF.denoise(emu, even, odd, r, f, 0.45)
        n = int((gpu.view(np.uint32) != cpu.view(np.uint32)).sum())
        print(f"r={r} f={f}: {n} of {gpu.size} words differ between the host emulation and the GPU (max abs {np.abs(gpu - cpu).max():.3e})")
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
    return films


RENDERED = [("cornell_box", ""), ("smallpt", ""), ("cornell_box", "wave")]


@pytest.mark.parametrize("name,mode", RENDERED, ids=["cornell_box", "smallpt", "cornell_box-wavefront"])
def test_rendered_films(name, mode, tmp_path, monkeypatch):
    if mode:
        monkeypatch.setenv("TRAYHIP_MODE", mode)
    w, h, spp = 160, 96, 32
    scene, *_ = load(getattr(scenes, name)(w, h, spp), tmp_path)
    hip = T.Hip(0, seed=7)
    even, odd = range_films(hip, scene, spp)
    assert hip.schedule(scene)["launched_wavefront"] == (1 if mode else 0), "TRAYHIP_MODE did not select the schedule"
    r, f, k = 7, 3, 0.45
    out = hip.denoise(even, odd, r, f, k)
    D.assert_matches(out, even, odd, r, f, k, f"{name} {mode or 'tiles'} 160x96x32")
    scene.release_device()
    ref = reference_image(scene, 4096, seed=1234)
    noisy, clean = rmse(rgb(even + odd), ref), rmse(out[..., :3], ref)
    print(f"{name} {mode or 'tiles'}: RMSE(even + odd) = {noisy:.5f}, RMSE(denoised) = {clean:.5f}, ratio {clean / noisy:.3f}")
    assert clean < noisy


def test_render_denoised_is_denoise_of_the_range_films(tmp_path):
    w, h, spp = 160, 96, 32
    scene, rt, _, fi = load(scenes.cornell_box(w, h, spp), tmp_path)
    cfg = T.Config(str(tmp_path), "s.json", spp, 1, fi)
    hip = T.Hip(0, seed=9)
    assert hip.render_denoised(scene, rt, cfg) is None
    got = rt.get_renderf32().reshape(h, w, 4)
    even, odd = range_films(T.Hip(0, seed=9), scene, spp)
    D.assert_matches(got, even, odd, 7, 3, 0.45, "render_denoised against the statement on the two range films")
    rt.clear()
    hip.render_denoised(scene, rt, cfg, radius=3, patch=1, k=1.0)
    D.assert_matches(rt.get_renderf32().reshape(h, w, 4), even, odd, 3, 1, 1.0, "render_denoised(radius=3, patch=1, k=1)")
    # torch tensors in, a torch tensor out
    import torch
    t = hip.denoise(torch.from_numpy(even).cuda(), torch.from_numpy(odd).cuda(), 3, 1, 1.0)
    assert isinstance(t, torch.Tensor) and t.is_cuda
    D.assert_matches(t.cpu().numpy(), even, odd, 3, 1, 1.0, "Hip.denoise of torch tensors")


@pytest.mark.parametrize("threshold", [0.0, 3.0e38], ids=["threshold-0", "huge-threshold"])
def test_render_denoised_with_a_threshold(threshold, tmp_path):
    """far from any tile's error the tile samples are decided the same way in every run: the films are those of a separate noise-target call"""
    import torch
    w, h, spp, lo = 160, 96, 32, 8
    scene, rt, _, fi = load(scenes.cornell_box(w, h, spp), tmp_path)
    cfg = T.Config(str(tmp_path), "s.json", spp, 1, fi)
    hip = T.Hip(0, seed=9)
    smp, err = hip.render_denoised(scene, rt, cfg, threshold=threshold, min_spp=lo)
    got = rt.get_renderf32().reshape(h, w, 4)
    dev = scene.device_scene(0, 0)
    even = torch.zeros(w * h * 4, dtype=torch.float32, device="cuda:0")
    odd = torch.zeros_like(even)
    n = len(T.BlockQueue((w, h), (8, 8)).blocks)
    smp_c, err_c = np.zeros(n, np.uint32), np.zeros(n, np.float32)
    T.check(T.lib().tray_render_noise_target_device(dev, 0, 0, lo, spp, threshold, 9, C.c_void_p(even.data_ptr()), C.c_void_p(odd.data_ptr()),
                                                    smp_c.ctypes.data_as(C.POINTER(C.c_uint32)), err_c.ctypes.data_as(C.POINTER(C.c_float)), None))
    torch.cuda.synchronize()
    assert (smp == smp_c).all() and (smp == (spp if threshold == 0.0 else lo)).all(), (smp, smp_c)
    even, odd = even.cpu().numpy().reshape(h, w, 4), odd.cpu().numpy().reshape(h, w, 4)
    D.assert_matches(got, even, odd, 7, 3, 0.45, f"render_denoised(threshold={threshold}) against the statement on a noise-target call's films")


def test_full_size_frame(tmp_path):
    """1920 x 1080, cornell_box at 64 spp through render_denoised: finite, the range property on a strided sample of blocks, and three 96 x 96
    crops (a corner, an edge, the centre; each cut with its r + f + 1 surroundings) against the f64 statement of the sub-image"""
    w, h, spp = 1920, 1080, 64
    r, f, k = 7, 3, 0.45
    scene, rt, _, fi = load(scenes.cornell_box(w, h, spp), tmp_path)
    cfg = T.Config(str(tmp_path), "s.json", spp, 1, fi)
    hip = T.Hip(0, seed=3)
    hip.render_denoised(scene, rt, cfg)
    got = rt.get_renderf32().reshape(h, w, 4)
    assert np.isfinite(got).all() and (got[..., 3] == 1.0).all()
    even, odd = range_films(T.Hip(0, seed=3), scene, spp)
    m = r + f + 1
    for what, (x0, y0) in [("corner", (0, 0)), ("edge", (w - 96, 500)), ("centre", (912, 492))]:
        xs0, ys0, xs1, ys1 = max(0, x0 - m), max(0, y0 - m), min(w, x0 + 96 + m), min(h, y0 + 96 + m)
        e, o = np.ascontiguousarray(even[ys0:ys1, xs0:xs1]), np.ascontiguousarray(odd[ys0:ys1, xs0:xs1])
        want, tol, err32, _ = D.bar(e, o, r, f, k)
        cut = (slice(y0 - ys0, y0 - ys0 + 96), slice(x0 - xs0, x0 - xs0 + 96))
        diff = np.abs(got[y0:y0 + 96, x0:x0 + 96, :3].astype(np.float64) - want[cut])
        print(f"1920x1080 {what} crop: kernels - f64 statement = {diff.max():.3e}, f32 statement - f64 statement = {err32:.3e}, bar {tol:.3e}")
        assert diff.max() <= tol, what
    # the range property inside 64 x 64 blocks on a stride, each cut with its r surroundings
    for y0 in range(0, h - 64, 250):
        for x0 in range(0, w - 64, 450):
            xs0, ys0, xs1, ys1 = max(0, x0 - r), max(0, y0 - r), min(w, x0 + 64 + r), min(h, y0 + 64 + r)
            e, o = even[ys0:ys1, xs0:xs1], odd[ys0:ys1, xs0:xs1]
            inner = np.zeros(e.shape[:2], bool)
            inner[y0 - ys0:y0 - ys0 + 64, x0 - xs0:x0 - xs0 + 64] = True
            inner &= D.resolve(e, o)[0]
            bad = D.range_violations(got[ys0:ys1, xs0:xs1, :3], e, o, r, where=inner)
            assert len(bad) == 0, (x0, y0, bad[:4].tolist())
