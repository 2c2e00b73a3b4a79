"""The albedo-demodulated temporal filter on the GPU (tray_denoise_temporal_demodulated_device, Hip.denoise_temporal(albedos=...),
Hip.render_sequence_denoised(demodulate=True)).

Every comparison is with the f64 numpy statement of the call computed on the host (tests/_tdemod_ref.py) under its bars: the temporal bar -- 4 x
what the f32 statement differs from the f64 one on the same films, plus 1e-7 -- times the largest s_0, and the same over the centre's valid
pixels. Small films whose every workgroup lies partly outside the image, the three identities of include/trayhip.h to the bit on the device, the
host emulation's bits, Python's entry point, a three-frame textured sequence rendered by the project, and a 1920 x 1080 call checked on a
crop. Two calls give the same bits, and guard bytes around the output and the scratch buffer stay intact. Nothing here reads the reference."""
import numpy as np
import pytest

import tray_rust_amd as T
import _denoise_ref as D
import _first_hit_ref as FH
import _tdemod_ref as TD
import _temporal_ref as TR
from _denoise_ref import rgb, rmse
from _tdemod_ref import same_bits, tdemod_guarded

pytestmark = pytest.mark.gpu

RTF = [(3, 2, 1), (10, 7, 3)]
IDS = [f"r{r}t{rt}f{f}" for r, rt, f in RTF]
K = 0.45


@pytest.mark.parametrize("r,rt,f", RTF, ids=IDS)
@pytest.mark.parametrize("w,h", [(9, 5), (33, 17), (67, 45)], ids=["9x5", "33x17", "67x45"])
def test_small_films_and_partial_workgroups(built, w, h, r, rt, f):
    """9 x 5: one workgroup, 33 x 17: four, each partly outside the image; 67 x 45: nine. N = 2."""
    frames = TD.random_frames(w, h, 3, seed=11 * w + h)
    out = tdemod_guarded(frames, r, rt, f, K)
    TD.assert_matches(out, frames, r, rt, f, K, f"gpu {w}x{h} r={r} rt={rt} f={f} N=2")
    assert same_bits(out, tdemod_guarded(frames, r, rt, f, K)), "two calls differ"
    cpu = TD.run(TD.tdemod_lib(), frames, r, rt, f, K)   # (builds the emulation when first called)
    n = int((out.view(np.uint32) != cpu.view(np.uint32)).sum())
    print(f"{w}x{h} r={r} rt={rt} f={f}: {n} of {out.size} words differ between the host emulation and the GPU (max abs {np.abs(out - cpu).max():.3e})")
    assert np.abs(out - cpu).max() <= 1e-5


@pytest.mark.parametrize("w,h", [(67, 45), (160, 96)], ids=["67x45", "160x96"])
def test_the_three_identities_hold_to_the_bit(built, w, h):
    r, rt, f = 7, 3, 3
    frames = TD.random_frames(w, h, 3, seed=7 * w + h)
    # (a) without neighbours: tray_denoise_demodulated_device with radius2 = 0
    got = tdemod_guarded(frames[:1], r, rt, f, K)
    want = FH.demodulated_guarded(*frames[0], r, f, K)
    assert same_bits(got, want), ("a", int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    # (b) albedo films without a valid pixel: tray_denoise_temporal_device
    pairs = [fr[:2] for fr in frames]
    want = TR.temporal_guarded(pairs, r, rt, f, K)
    for kind in ("zero-weight", "nan", "negative-weight"):
        got = tdemod_guarded([(e, o, TD.weightless_albedo(kind, w, h)) for e, o in pairs], r, rt, f, K)
        assert same_bits(got, want), ("b", kind, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    # (c) in general: numpy-f32 demodulation, tray_denoise_temporal_device, numpy-f32 remodulation
    got = tdemod_guarded(frames, r, rt, f, K)
    want = TD.composed(lambda quotients: TR.temporal_guarded(quotients, r, rt, f, K), frames)
    assert same_bits(got, want), ("c", int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    assert not same_bits(got, TR.temporal_guarded(pairs, r, rt, f, K))


def test_python_gives_the_c_calls_bits(built):
    import torch
    w, h, (r, rt, f) = 67, 45, (7, 3, 3)
    frames = TD.random_frames(w, h, 3, seed=4)
    want = tdemod_guarded(frames, r, rt, f, K)
    hip = T.Hip(0)
    order = [frames[1], frames[0], frames[2]]   # the centre in the middle, the neighbours in list order
    got = hip.denoise_temporal([fr[:2] for fr in order], 1, r, rt, f, K, albedos=[fr[2] for fr in order])
    assert isinstance(got, np.ndarray) and same_bits(got, want)
    dev = [tuple(torch.from_numpy(x).cuda() for x in fr) for fr in order]
    t = hip.denoise_temporal([fr[:2] for fr in dev], 1, r, rt, f, K, albedos=[fr[2] for fr in dev])
    assert isinstance(t, torch.Tensor) and t.is_cuda and same_bits(t.cpu().numpy(), want)
    one = hip.denoise_temporal([frames[0][:2]], 0, r, rt, f, K, albedos=[frames[0][2]])
    assert same_bits(one, hip.denoise(*frames[0][:2], r, f, K, albedo=frames[0][2]))


W, H, SPP = 160, 96, 32


def test_a_rendered_textured_sequence(tmp_path):
    """textured_box over three frames at 160 x 96, 32 spp: the image render_sequence_denoised(demodulate=True, reach=1) yields for frame 1 is
    denoise_temporal(albedos=...) of the very films it rendered (read at the filter's call: a film is a sum of float atomics, so a second render
    need not give the same bits), every albedo film is rendered once, and against a 4096-spp render of frame 1 with another seed the image
    beats both existing calls on the same films, which beat the plain filter, which beats the noisy frame."""
    import torch
    scene, rt_, _, fi = TD.textured_sequence(str(tmp_path), W, H, SPP)
    cfg = T.Config(str(tmp_path), "textured_box.json", SPP, 1, fi)
    hip = T.Hip(0, seed=9)
    albedo_renders, filtered = [], []
    first_hit, filt = hip.render_first_hit_device, hip._denoise_temporal_device

    def first_hit_spy(scene_, frame, select_blocks, spp, rng, *a, **kw):
        albedo_renders.append((int(frame), tuple(int(v) for v in rng), int(spp)))
        return first_hit(scene_, frame, select_blocks, spp, rng, *a, **kw)

    def filter_spy(centre, neighbours, radius, radius_t, patch, k, albedos):
        torch.cuda.synchronize()
        filtered.append(([tuple(x.cpu().numpy() for x in pair) for pair in [centre] + list(neighbours)], [a.cpu().numpy() for a in albedos]))
        return filt(centre, neighbours, radius, radius_t, patch, k, albedos)

    hip.render_first_hit_device, hip._denoise_temporal_device = first_hit_spy, filter_spy
    got = list(hip.render_sequence_denoised(scene, cfg, range(3), reach=1, demodulate=True))
    assert [f for f, _ in got] == [0, 1, 2]
    assert sorted(albedo_renders) == [(g, (0, SPP), SPP) for g in range(3)], albedo_renders   # each once
    assert [len(pairs) for pairs, _ in filtered] == [2, 3, 2]
    other = T.Hip(0, seed=9)
    for (f, img), (pairs, albedos) in zip(got, filtered):
        want = other.denoise_temporal(pairs, 0, albedos=albedos)
        assert img.shape == (H, W, 4) and same_bits(img, want), f
    pairs, albedos = filtered[1]   # frame 1, then frames 0 and 2
    for g, a in zip((0, 2), albedos[1:]):
        print(f"resolved albedo of frame {g} differs from frame 1's by RMSE {rmse(rgb(a), rgb(albedos[0])):.3f}")
    both = got[1][1]
    TD.assert_matches(both, [p + (a,) for p, a in zip(pairs, albedos)], 7, 3, 3, K, "render_sequence_denoised(demodulate=True), frame 1")
    even, odd = pairs[0]
    plain = other.denoise(even, odd)
    demod = other.denoise(even, odd, albedo=albedos[0])
    temporal = other.denoise_temporal(pairs, 0)
    scene.release_device()
    film = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0")
    T.Hip(0, seed=1234).render_device(scene, 1, (0, 0), 4096, film.data_ptr())
    torch.cuda.synchronize()
    ref = rgb(film.cpu().numpy().reshape(H, W, 4))
    e = [rmse(x, ref) for x in (rgb(even + odd), plain[..., :3], demod[..., :3], temporal[..., :3], both[..., :3])]
    print(f"textured_box {W}x{H} {SPP} spp, frames 0 - 2: RMSE(noisy) = {e[0]:.5f}, RMSE(plain) = {e[1]:.5f}, RMSE(demodulated) = {e[2]:.5f}, "
          f"RMSE(temporal) = {e[3]:.5f}, RMSE(temporal + demodulated) = {e[4]:.5f}: {e[4] / min(e[2], e[3]):.3f} x the better of the two, "
          f"{e[4] / e[1]:.3f} x the plain filter")
    assert e[4] < min(e[2], e[3]) < e[1] < e[0]


def test_full_size_call(tmp_path):
    """1920 x 1080, textured_box range films and albedo films of three seeds as three frames, N = 2 and the defaults: finite, weight 1, and one
    96 x 96 crop (cut with its r + f + 1 surroundings) against the f64 statement of the sub-images"""
    import torch
    from tray_rust_amd import scenes
    w, h, spp = 1920, 1080, 16
    r, rt, f = 7, 3, 3
    scene = T.Scene.load_file(scenes.write_textured_box(str(tmp_path), width=w, height=h, samples=spp))[0]
    frames = []
    for seed in (3, 4, 5):
        hip = T.Hip(0, seed=seed)
        films = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0") for _ in range(5)]
        for film, rng in zip(films, ((0, spp // 2), (spp // 2, spp))):
            hip.render_samples_device(scene, 0, (0, 0), spp, rng, film.data_ptr())
        hip.render_first_hit_device(scene, 0, (0, 0), spp, (0, spp), *[t.data_ptr() for t in films[2:]])
        torch.cuda.synchronize()
        frames.append(tuple(t.cpu().numpy() for t in films[:3]))
    got = T.Hip(0).denoise_temporal([fr[:2] for fr in frames], 0, albedos=[fr[2] for fr in frames])
    assert np.isfinite(got).all() and (got[..., 3] == 1.0).all()
    m = r + f + 1
    x0, y0 = 912, 492
    xs0, ys0, xs1, ys1 = x0 - m, y0 - m, x0 + 96 + m, y0 + 96 + m
    cut_frames = [tuple(np.ascontiguousarray(x[ys0:ys1, xs0:xs1]) for x in fr) for fr in frames]
    want, tol, err32, _ = TD.bar(cut_frames, r, rt, f, K)
    diff = np.abs(got[y0:y0 + 96, x0:x0 + 96, :3].astype(np.float64) - want[m:m + 96, m:m + 96])
    print(f"1920x1080 centre crop: kernels - f64 statement = {diff.max():.3e}, f32 statement - f64 statement = {err32:.3e}, bar {tol:.3e}")
    assert diff.max() <= tol
