"""The two-pass temporal filter on the GPU (tray_denoise_temporal_halves_device, tray_denoise_temporal_guided_device,
tray_denoise_temporal_two_pass_device, Hip.denoise_temporal(passes=2), Hip.render_sequence_denoised(passes=2)).

Every comparison is with the f64 numpy statements of the calls computed on the host (tests/_temporal2_ref.py) under their bars: 4 x what the f32
statement differs from the f64 one on the same films, plus 1e-7, over the whole image and over the centre's valid pixels. Small films whose every
workgroup lies partly outside the image, the host emulation's bits (0 words differ), the five identities of include/trayhip.h and the two-pass
call's composition to the bit against the existing calls on the device, Python's entry points, a three-frame textured sequence rendered by the
project, and a 1920 x 1080 call checked on a crop. Two calls give the same bits, and guard bytes around the outputs and the scratch buffer stay
intact. Nothing here reads the reference."""
import numpy as np
import pytest

import tray_rust_amd as T
import _guided_ref as G
import _tdemod_ref as TD
import _temporal_ref as TR
import _temporal2_ref as T2
from _denoise_ref import resolve, rgb, rmse
from _temporal2_ref import guided_guarded, halves_guarded, same_bits, two_pass_guarded

pytestmark = pytest.mark.gpu

RTF = [(3, 2, 1), (10, 7, 3)]
IDS = [f"r{r}t{rt}f{f}" for r, rt, f in RTF]
K = 0.45
R2, RT2, F2, K2 = T2.DEFAULTS2


def differing(a, b):
    return int((np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32)).sum())


@pytest.mark.parametrize("r,rt,f", RTF, ids=IDS)
@pytest.mark.parametrize("w,h", [(9, 5), (33, 17), (67, 45)], ids=["9x5", "33x17", "67x45"])
def test_small_films_and_partial_workgroups(built, w, h, r, rt, f):
    """9 x 5: one workgroup, 33 x 17: four, each partly outside the image; 67 x 45: nine. N = 2; pass 1 at (r, rt, f), pass 2 at (5, 3, 1). The
    guided call is made at pass 1's parameters too, with guides of other seeds."""
    seed = 11 * w + h
    frames = TR.random_frames(w, h, 3, seed=seed)
    guides = T2.random_guides(w, h, 3, seed=seed)
    emu = T2.temporal2_lib()   # (builds the emulation when first called)
    what = f"gpu {w}x{h} r={r} rt={rt} f={f} N=2"
    fa, fb = halves_guarded(frames, r, rt, f, K)
    T2.assert_halves(fa, fb, frames, r, rt, f, K, what + " halves")
    out_g = guided_guarded(frames, guides, r, rt, f, K2)
    T2.assert_guided(out_g, frames, guides, r, rt, f, K2, what + " guided")
    out_2 = two_pass_guarded(frames, r, rt, f, K, R2, RT2, F2, K2)
    T2.assert_two_pass(out_2, frames, r, rt, f, K, R2, RT2, F2, K2, what + " two-pass")
    again = halves_guarded(frames, r, rt, f, K) + (guided_guarded(frames, guides, r, rt, f, K2), two_pass_guarded(frames, r, rt, f, K, R2, RT2, F2, K2))
    cpu = T2.run_halves(emu, frames, r, rt, f, K) + (T2.run_guided(emu, frames, guides, r, rt, f, K2), T2.run_two_pass(emu, frames, r, rt, f, K, R2, RT2, F2, K2))
    for name, got, second, host in zip(("fa", "fb", "guided", "two-pass"), (fa, fb, out_g, out_2), again, cpu):
        assert same_bits(got, second), f"{name}: two calls differ"
        n = differing(got, host)
        print(f"{what} {name}: {n} of {got.size} words differ between the host emulation and the GPU")
        assert n == 0, name


@pytest.mark.parametrize("w,h", [(67, 45), (160, 96)], ids=["67x45", "160x96"])
def test_the_identities_and_the_composition_hold_to_the_bit(built, w, h):
    r, rt, f = 7, 3, 3
    frames = TR.random_frames(w, h, 3, seed=7 * w + h)
    guides = T2.random_guides(w, h, 3, seed=7 * w + h)
    hip = T.Hip(0)
    temporal = TR.temporal_guarded(frames, r, rt, f, K)
    # the halves' mean is the temporal call
    fa, fb = halves_guarded(frames, r, rt, f, K)
    mean = ((fa[..., :3] + fb[..., :3]) * np.float32(0.5)).astype(np.float32)
    assert same_bits(mean, temporal[..., :3]), ("mean", differing(mean, temporal[..., :3]))
    # the halves without neighbours are tray_denoise_halves_device's
    own = [hip.denoise_halves(e, o, r, f, K) for e, o in frames]
    got = halves_guarded(frames[:1], r, rt, f, K)
    assert all(same_bits(x, y) for x, y in zip(got, own[0])), ("halves N = 0", [differing(x, y) for x, y in zip(got, own[0])])
    # (i) guided by its own frames (the guide pointers are the films'): the temporal call
    got = guided_guarded(frames, frames, r, rt, f, K)
    assert same_bits(got, temporal), ("i", differing(got, temporal))
    # (ii) without neighbours: tray_denoise_guided_device
    got = guided_guarded(frames[:1], guides[:1], R2, RT2, F2, K2)
    want = G.guided_guarded(*frames[0], *guides[0], R2, F2, K2)
    assert same_bits(got, want), ("ii", differing(got, want))
    # the two-pass call without neighbours: tray_denoise_two_pass_device
    got = two_pass_guarded(frames[:1], r, rt, f, K, R2, RT2, F2, K2)
    want = G.two_pass_guarded(*frames[0], r, f, K, R2, F2, K2)
    assert same_bits(got, want), ("two-pass N = 0", differing(got, want))
    # the two-pass call is its composition: the centre's halves over all frames, every neighbour's own halves, the guided call
    got = two_pass_guarded(frames, r, rt, f, K, R2, RT2, F2, K2)
    want = guided_guarded(frames, [(fa, fb)] + own[1:], R2, RT2, F2, K2)
    assert same_bits(got, want), ("composition", differing(got, want))
    assert not same_bits(got, temporal)


def test_python_gives_the_c_calls_bits(built):
    import torch
    w, h, (r, rt, f) = 67, 45, (7, 3, 3)
    frames = TR.random_frames(w, h, 3, seed=4)
    guides = T2.random_guides(w, h, 3, seed=4)
    second = dict(radius2=R2, radius_t2=RT2, patch2=F2, k2=K2)
    want = two_pass_guarded(frames, r, rt, f, K, R2, RT2, F2, K2)
    want_h = halves_guarded(frames, r, rt, f, K)
    want_g = guided_guarded(frames, guides, R2, RT2, F2, K2)
    hip = T.Hip(0)
    order = lambda x: [x[1], x[0], x[2]]   # the centre in the middle, the neighbours in list order
    got = hip.denoise_temporal(order(frames), 1, r, rt, f, K, passes=2, **second)
    assert isinstance(got, np.ndarray) and same_bits(got, want)
    assert same_bits(hip.denoise_temporal(order(frames), 1, r, rt, f, K, passes=2), want)   # the defaults are (5, 3, 1, 1.0)
    got_h = hip.denoise_temporal_halves(order(frames), 1, r, rt, f, K)
    assert all(isinstance(x, np.ndarray) and same_bits(x, y) for x, y in zip(got_h, want_h))
    assert same_bits(hip.denoise_temporal_guided(order(frames), order(guides), 1), want_g)
    up = lambda prs: [tuple(torch.from_numpy(x).cuda() for x in pr) for pr in prs]
    dev, gdev = up(order(frames)), up(order(guides))
    t = hip.denoise_temporal(dev, 1, r, rt, f, K, passes=2, **second)
    assert isinstance(t, torch.Tensor) and t.is_cuda and same_bits(t.cpu().numpy(), want)
    th = hip.denoise_temporal_halves(dev, 1, r, rt, f, K)
    assert all(isinstance(x, torch.Tensor) and same_bits(x.cpu().numpy(), y) for x, y in zip(th, want_h))
    assert same_bits(hip.denoise_temporal_guided(dev, gdev, 1).cpu().numpy(), want_g)
    one = hip.denoise_temporal(frames[:1], 0, r, rt, f, K, passes=2)
    assert same_bits(one, hip.denoise(*frames[0], r, f, K, passes=2))


W, H, SPP = 160, 96, 32


def test_a_rendered_textured_sequence(tmp_path):
    """textured_box over three frames at 160 x 96, 32 spp: the image render_sequence_denoised(passes=2, reach=1) yields for every frame is
    denoise_temporal(passes=2) of the very films it rendered (read at the filter's call: a film is a sum of float atomics, so a second render
    need not give the same bits), every frame's own first-pass halves are computed once, and against a 4096-spp render of frame 1 with another
    seed the image beats the temporal call on the same films."""
    import torch
    scene, rt_, _, fi = TD.textured_sequence(str(tmp_path), W, H, SPP)
    cfg = T.Config(str(tmp_path), "textured_box.json", SPP, 1, fi)
    hip = T.Hip(0, seed=9)
    own_halves, filtered = [], []
    single, pilot = hip._denoise_halves_device, hip._denoise_temporal_halves_device

    def single_spy(e, o, *a):
        own_halves.append(e.data_ptr())
        return single(e, o, *a)

    def pilot_spy(centre, neighbours, *a):
        torch.cuda.synchronize()
        filtered.append([tuple(x.cpu().numpy() for x in pair) for pair in [centre] + list(neighbours)])
        return pilot(centre, neighbours, *a)

    hip._denoise_halves_device, hip._denoise_temporal_halves_device = single_spy, pilot_spy
    got = list(hip.render_sequence_denoised(scene, cfg, range(3), reach=1, passes=2))
    assert [f for f, _ in got] == [0, 1, 2]
    assert len(own_halves) == 3 and len(set(own_halves)) == 3, own_halves   # each frame's once, every frame in films of its own
    assert [len(pairs) for pairs in filtered] == [2, 3, 2]
    other = T.Hip(0, seed=9)
    for (f, img), pairs in zip(got, filtered):
        want = other.denoise_temporal(pairs, 0, passes=2)
        assert img.shape == (H, W, 4) and same_bits(img, want), (f, differing(img, want))
    pairs = filtered[1]   # frame 1, then frames 0 and 2
    both = got[1][1]
    T2.assert_two_pass(both, pairs, 7, 3, 3, K, R2, RT2, F2, K2, "render_sequence_denoised(passes=2), frame 1")
    even, odd = pairs[0]
    plain = other.denoise(even, odd)
    alone = other.denoise(even, odd, passes=2)
    temporal = other.denoise_temporal(pairs, 0)
    scene.release_device()
    film = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0")
    T.Hip(0, seed=1234).render_device(scene, 1, (0, 0), 4096, film.data_ptr())
    torch.cuda.synchronize()
    ref = rgb(film.cpu().numpy().reshape(H, W, 4))
    e = [rmse(x, ref) for x in (rgb(even + odd), plain[..., :3], alone[..., :3], temporal[..., :3], both[..., :3])]
    print(f"textured_box {W}x{H} {SPP} spp, frames 0 - 2: RMSE(noisy) = {e[0]:.5f}, RMSE(plain) = {e[1]:.5f}, RMSE(two-pass, one frame) = {e[2]:.5f}, "
          f"RMSE(temporal) = {e[3]:.5f}, RMSE(two-pass temporal) = {e[4]:.5f}: {e[4] / e[3]:.3f} x the temporal call, {e[4] / e[2]:.3f} x the single-frame "
          f"two-pass call, {e[4] / e[1]:.3f} x the plain filter")
    assert e[4] < e[3]


def test_full_size_call(built):
    """1920 x 1080 generator films, N = 2 and the defaults: finite, weight 1, and one 96 x 96 crop (cut with the surroundings both passes reach:
    r + f + 1 of the pilots and r2 + f2 + 1 of the second pass) against the f64 statement of the sub-images"""
    w, h = 1920, 1080
    r, rt, f = 7, 3, 3
    frames = TR.random_frames(w, h, 3, seed=21)
    got = T.Hip(0).denoise_temporal(frames, 0, passes=2)
    assert np.isfinite(got).all() and (got[..., 3] == 1.0).all()
    m = (r + f + 1) + (R2 + F2 + 1)
    x0, y0 = 912, 492   # (the generator's colour edge at x = 960 runs through the crop)
    xs0, ys0, xs1, ys1 = x0 - m, y0 - m, x0 + 96 + m, y0 + 96 + m
    cut = [tuple(np.ascontiguousarray(x[ys0:ys1, xs0:xs1]) for x in fr) for fr in frames]
    want, f32 = (T2.two_pass(cut, r, rt, f, K, R2, RT2, F2, K2, F)[m:m + 96, m:m + 96] for F in (np.float64, np.float32))
    err32 = float(np.abs(f32.astype(np.float64) - want).max())   # the bar of the crop's own pixels
    tol = 4.0 * err32 + 1e-7
    diff = np.abs(got[y0:y0 + 96, x0:x0 + 96, :3].astype(np.float64) - want)
    print(f"1920x1080 centre crop: kernels - f64 statement = {diff.max():.3e}, f32 statement - f64 statement = {err32:.3e}, bar {tol:.3e}")
    assert diff.max() <= tol
