"""The temporal NL-means filter on the GPU (tray_denoise_temporal_device, Hip.denoise_temporal, Hip.render_sequence_denoised).

Every comparison is with the f64 numpy statement of the filter computed on the host (tests/_temporal_ref.py) under its bar: 4 x what the f32
statement differs from the f64 one on the same films, plus 1e-7. The generator films (invalid pixels of every kind) with two neighbours, one
frame against tray_denoise_device's bits, the host emulation's bits as a finding, three frames of a moving scene rendered by the tile kernel
and by the wavefront schedule, the sequence generator against separately rendered films, and a 1920 x 1080 call checked on crops. Two calls
give the same bits, and guard bytes around the output and the scratch buffer stay intact. Nothing here reads the reference."""
import numpy as np
import pytest

import tray_rust_amd as T
from tray_rust_amd import scenes
import _denoise_ref as D
import _temporal_ref as TR
from _denoise_ref import denoise_guarded, rgb, rmse
from _noise_ref import load
from _temporal_ref import temporal_guarded

pytestmark = pytest.mark.gpu

RTF = [(1, 1, 0), (3, 2, 1), (7, 3, 3), (10, 7, 3)]
RF = [(1, 0), (3, 1), (7, 3), (10, 3)]


@pytest.mark.parametrize("r,rt,f", RTF, ids=[f"r{r}t{rt}f{f}" for r, rt, f in RTF])
@pytest.mark.parametrize("w,h", [(67, 45), (160, 96)], ids=["67x45", "160x96"])
def test_generator_films_match_the_f64_statement(built, w, h, r, rt, f):
    frames = TR.random_frames(w, h, 3, seed=11 * w + h)
    out = temporal_guarded(frames, r, rt, f, 0.45)
    TR.assert_matches(out, frames, r, rt, f, 0.45, f"gpu {w}x{h} r={r} rt={rt} f={f} N=2")
    again = temporal_guarded(frames, r, rt, f, 0.45)
    assert (out.view(np.uint32) == again.view(np.uint32)).all(), "two calls differ"
    assert len(TR.range_violations(out[..., :3], frames, r, rt)) == 0
    via_python = T.Hip(0).denoise_temporal([frames[1], frames[0], frames[2]], 1, r, rt, f, 0.45)
    assert isinstance(via_python, np.ndarray) and (via_python.view(np.uint32) == out.view(np.uint32)).all()


@pytest.mark.parametrize("r,f", RF, ids=[f"r{r}f{f}" for r, f in RF])
def test_one_frame_gives_tray_denoise_devices_bits(built, r, f):
    for w, h in [(67, 45), (160, 96)]:
        even, odd = D.random_films(w, h, seed=11 * w + h)
        want = denoise_guarded(even, odd, r, f, 0.45)
        got = temporal_guarded([(even, odd)], r, 1, f, 0.45)
        assert (got.view(np.uint32) == want.view(np.uint32)).all(), (w, h, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    via_python = T.Hip(0).denoise_temporal([(even, odd)], 0, r, 1, f, 0.45)
    assert (via_python.view(np.uint32) == T.Hip(0).denoise(even, odd, r, f, 0.45).view(np.uint32)).all()


def test_emulation_and_gpu_bits(built):
    """a finding, not a requirement: with tr::ref_expf on both sides and IEEE division the host emulation is expected to give the GPU's bits"""
    frames = TR.random_frames(67, 45, 3, seed=5)
    emu = TR.temporal_lib()   # (builds the emulation when called, here only)
    for r, rt, f in RTF:
        gpu = temporal_guarded(frames, r, rt, f, 0.45)
        cpu = TR.run(emu, frames, r, rt, f, 0.45)
        n = int((gpu.view(np.uint32) != cpu.view(np.uint32)).sum())
        print(f"r={r} rt={rt} f={f}: {n} of {gpu.size} words differ between the host emulation and the GPU (max abs {np.abs(gpu - cpu).max():.3e})")
        assert np.abs(gpu - cpu).max() <= 1e-5


def range_films(hip, scene, frame, spp):
    """the films of [0, spp / 2) and [spp / 2, spp) of a frame, rendered separately"""
    import torch
    fl = scene.flatten(frame).contents.film
    w, h = fl.width, fl.height
    films = []
    for rng in ((0, spp // 2), (spp // 2, spp)):
        film = torch.zeros(w * h * 4, dtype=torch.float32, device="cuda:0")
        hip.render_samples_device(scene, frame, (0, 0), spp, rng, film.data_ptr())
        torch.cuda.synchronize()
        films.append(film.cpu().numpy().reshape(h, w, 4))
    return tuple(films)


W, H, SPP, FRAMES, CENTRE = 160, 96, 32, 48, 24


@pytest.mark.parametrize("mode", ["", "wave"], ids=["tiles", "wavefront"])
def test_rendered_films(mode, tmp_path, monkeypatch):
    if mode:
        monkeypatch.setenv("TRAYHIP_MODE", mode)
    scene, *_ = load(scenes.moving_box(W, H, SPP, frames=FRAMES), tmp_path)
    hip = T.Hip(0, seed=7)
    pairs = {g: range_films(hip, scene, g, SPP) for g in (CENTRE - 1, CENTRE, CENTRE + 1)}
    assert hip.schedule(scene)["launched_wavefront"] == (1 if mode else 0), "TRAYHIP_MODE did not select the schedule"
    r, rt, f, k = 7, 3, 3, 0.45
    frames = [pairs[CENTRE], pairs[CENTRE - 1], pairs[CENTRE + 1]]
    out = hip.denoise_temporal([pairs[CENTRE - 1], pairs[CENTRE], pairs[CENTRE + 1]], 1, r, rt, f, k)
    TR.assert_matches(out, frames, r, rt, f, k, f"moving_box {mode or 'tiles'} {W}x{H}x{SPP}, frames 23 - 25")
    spatial = hip.denoise(*pairs[CENTRE], r, f, k)
    scene.release_device()
    import torch
    fl = scene.flatten(CENTRE).contents.film
    film = torch.zeros(fl.width * fl.height * 4, dtype=torch.float32, device="cuda:0")
    T.Hip(0, seed=1234).render_device(scene, CENTRE, (0, 0), 4096, film.data_ptr())
    torch.cuda.synchronize()
    ref = rgb(film.cpu().numpy().reshape(H, W, 4))
    noisy, one, three = rmse(rgb(pairs[CENTRE][0] + pairs[CENTRE][1]), ref), rmse(spatial[..., :3], ref), rmse(out[..., :3], ref)
    print(f"moving_box {mode or 'tiles'}: RMSE(noisy) = {noisy:.5f}, RMSE(spatial) = {one:.5f}, RMSE(temporal) = {three:.5f}")
    assert three < one < noisy


def test_render_sequence_denoised_is_denoise_temporal_of_the_range_films(tmp_path):
    """Frames 22 - 26 with reach = 1: every frame's two range films are rendered once, each frame is filtered with its one or two neighbours in
    ascending order, and the image it yields is denoise_temporal of those films, bit for bit. A film is a sum of float atomics
    (include/trayhip.h), so two renders of one range need not be the same bits, and against separately rendered films the images did differ on
    the GPU (the number of film words that differ is printed): the bit comparison is therefore made on the very films the generator
    rendered, read at the filter's call, and these are compared with separately rendered films
    under tests/test_gpu_sample_ranges.py's bar for two renders of the same samples, 2e-5 of the film's largest value; the middle frame's image
    is also held against the statement on the separately rendered films, as test_gpu_denoise does for render_denoised."""
    scene, rt, _, fi = load(scenes.moving_box(W, H, SPP, frames=FRAMES), tmp_path)
    cfg = T.Config(str(tmp_path), "s.json", SPP, 1, fi)
    hip = T.Hip(0, seed=9)
    rendered, filtered = [], []
    render, filt = hip.render_samples_device, hip._denoise_temporal_device

    def render_spy(scene_, frame, select_blocks, spp, rng, *a, **kw):
        rendered.append((int(frame), tuple(int(v) for v in rng), int(spp)))
        return render(scene_, frame, select_blocks, spp, rng, *a, **kw)

    def filter_spy(centre, neighbours, *a):
        import torch
        torch.cuda.synchronize()
        filtered.append([tuple(x.cpu().numpy() for x in pair) for pair in [centre] + list(neighbours)])
        return filt(centre, neighbours, *a)

    hip.render_samples_device, hip._denoise_temporal_device = render_spy, filter_spy
    got = list(hip.render_sequence_denoised(scene, cfg, range(22, 27), reach=1))
    assert [f for f, _ in got] == [22, 23, 24, 25, 26]
    assert sorted(rendered) == sorted((g, rng, SPP) for g in range(22, 27) for rng in ((0, SPP // 2), (SPP // 2, SPP))), rendered   # each once
    other = T.Hip(0, seed=9)
    pairs = {g: range_films(other, scene, g, SPP) for g in range(22, 27)}
    for (f, img), films in zip(got, filtered):
        window = [f] + [g for g in (f - 1, f + 1) if 22 <= g <= 26]   # the centre, then the neighbours in ascending order
        assert len(films) == len(window) == (2 if f in (22, 26) else 3)
        want = other.denoise_temporal(films, 0)
        assert img.shape == (H, W, 4) and (img.view(np.uint32) == want.view(np.uint32)).all(), f
        for g, pair in zip(window, films):
            for mine, separate in zip(pair, pairs[g]):
                scale = max(1.0, float(np.abs(separate).max()))
                d, n = float(np.abs(mine - separate).max()), int((mine.view(np.uint32) != separate.view(np.uint32)).sum())
                print(f"frame {f}, films of frame {g}: {n} of {mine.size} words differ from a separate render, max {d:.2e} (bar {2e-5 * scale:.2e})")
                assert d <= 2e-5 * scale, (f, g)
    window = [pairs[24], pairs[23], pairs[25]]
    TR.assert_matches(got[2][1], window, 7, 3, 3, 0.45, "render_sequence_denoised, frame 24, against the statement on separately rendered films")
    # torch tensors in, a torch tensor out
    import torch
    t = other.denoise_temporal([tuple(torch.from_numpy(x).cuda() for x in pairs[g]) for g in (23, 24)], 1)
    assert isinstance(t, torch.Tensor) and t.is_cuda
    assert (t.cpu().numpy().view(np.uint32) == other.denoise_temporal([pairs[23], pairs[24]], 1).view(np.uint32)).all()


def test_full_size_call(tmp_path):
    """1920 x 1080, cornell_box range films of three seeds as three frames, N = 2 and the defaults: finite, weight 1, and three 96 x 96 crops (a
    corner, an edge, the centre; each cut with its r + f + 1 surroundings) against the f64 statement of the sub-images"""
    w, h, spp = 1920, 1080, 16
    r, rt, f, k = 7, 3, 3, 0.45
    scene, *_ = load(scenes.cornell_box(w, h, spp), tmp_path)
    frames = [range_films(T.Hip(0, seed=s), scene, 0, spp) for s in (3, 4, 5)]
    got = T.Hip(0).denoise_temporal(frames, 0)
    assert np.isfinite(got).all() and (got[..., 3] == 1.0).all()
    m = r + f + 1
    for what, (x0, y0) in [("corner", (0, 0)), ("edge", (w - 96, 500)), ("centre", (912, 492))]:
        xs0, ys0, xs1, ys1 = max(0, x0 - m), max(0, y0 - m), min(w, x0 + 96 + m), min(h, y0 + 96 + m)
        cut_frames = [tuple(np.ascontiguousarray(x[ys0:ys1, xs0:xs1]) for x in fr) for fr in frames]
        want, tol, err32, _ = TR.bar(cut_frames, r, rt, f, k)
        cut = (slice(y0 - ys0, y0 - ys0 + 96), slice(x0 - xs0, x0 - xs0 + 96))
        diff = np.abs(got[y0:y0 + 96, x0:x0 + 96, :3].astype(np.float64) - want[cut])
        print(f"1920x1080 {what} crop: kernels - f64 statement = {diff.max():.3e}, f32 statement - f64 statement = {err32:.3e}, bar {tol:.3e}")
        assert diff.max() <= tol, what
