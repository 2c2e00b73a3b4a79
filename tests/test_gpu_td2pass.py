"""The two-pass temporal filter on albedo-demodulated films on the GPU (tray_denoise_temporal_demodulated_halves_device, _guided_device,
_two_pass_device, Hip.denoise_temporal_demodulated, Hip.render_sequence_demodulated).

Every comparison is with the f64 numpy statements of the calls computed on the host (tests/_td2pass_ref.py) under their bars: 4 x what the f32
statement differs from the f64 one on the same films, plus 1e-7, times the largest s_0 where the output is remodulated, over the whole image
and over the centre's valid pixels. 9 x 5 is one workgroup and 33 x 17 four, each partly outside the image -- where the new kernel's end, which
loads the centre's albedo after the last barrier, can go wrong --, 67 x 45 nine; N = 0, 1, 2. The host emulation's bits, the four identities of
include/trayhip.h to the bit on the device, Python's entry points, and a three-frame textured sequence rendered by the project. Two calls give
the same bits, and guard bytes around the outputs and the scratch buffer stay intact. Nothing here reads the reference."""
import numpy as np
import pytest

import tray_rust_amd as T
import _first_hit_ref as FH
import _td2pass_ref as X
import _tdemod_ref as TD
import _temporal2_ref as T2
from _td2pass_ref import guided_guarded, halves_guarded, same_bits, two_pass_guarded

pytestmark = pytest.mark.gpu

K = 0.45
R2, RT2, F2, K2 = X.DEFAULTS2
# (w, h, N, first pass): the guided call is also made at the first pass's parameters, so that k_td2_guided_pass runs at every patch radius
CASES = [(9, 5, 0, (1, 1, 0)), (9, 5, 1, (3, 2, 2)), (9, 5, 2, (7, 3, 3)), (33, 17, 0, (3, 2, 2)), (33, 17, 1, (7, 3, 3)), (33, 17, 2, (1, 1, 0)),
         (67, 45, 2, (10, 7, 3))]


def differing(a, b):
    return int((np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32)).sum())


@pytest.mark.parametrize("w,h,n,rtf", CASES, ids=[f"{w}x{h}-N{n}-r{r}t{rt}f{f}" for w, h, n, (r, rt, f) in CASES])
def test_small_films_and_partial_workgroups(built, w, h, n, rtf):
    r, rt, f = rtf
    seed = 11 * w + h
    frames = TD.random_frames(w, h, n + 1, seed=seed)
    guides = X.random_guides(w, h, n + 1, seed=seed)
    emu = X.td2pass_lib()   # (builds the emulation when first called)
    what = f"gpu {w}x{h} r={r} rt={rt} f={f} N={n}"
    fa, fb = halves_guarded(frames, r, rt, f, K)
    X.assert_halves(fa, fb, frames, r, rt, f, K, what + " halves")
    out_g = guided_guarded(frames, guides, r, rt, f, K2)
    X.assert_guided(out_g, frames, guides, r, rt, f, K2, what + " guided")
    out_2 = two_pass_guarded(frames, r, rt, f, K, R2, RT2, F2, K2)
    X.assert_two_pass(out_2, frames, r, rt, f, K, R2, RT2, F2, K2, what + " two-pass")
    again = halves_guarded(frames, r, rt, f, K) + (guided_guarded(frames, guides, r, rt, f, K2), two_pass_guarded(frames, r, rt, f, K, R2, RT2, F2, K2))
    cpu = X.run_halves(emu, frames, r, rt, f, K) + (X.run_guided(emu, frames, guides, r, rt, f, K2), X.run_two_pass(emu, frames, r, rt, f, K, R2, RT2, F2, K2))
    for name, got, second, host in zip(("fa", "fb", "guided", "two-pass"), (fa, fb, out_g, out_2), again, cpu):
        assert same_bits(got, second), f"{name}: two calls differ"
        print(f"{what} {name}: {differing(got, host)} of {got.size} words differ between the host emulation and the GPU "
              f"(max abs {np.abs(got - host).max():.3e})")
        assert np.abs(got - host).max() <= 1e-5, name


@pytest.mark.parametrize("w,h,n", [(33, 17, 1), (67, 45, 2)], ids=["33x17-N1", "67x45-N2"])
def test_the_four_identities_hold_to_the_bit(built, w, h, n):
    r, rt, f = 7, 3, 3
    frames = TD.random_frames(w, h, n + 1, seed=7 * w + h)
    second = (R2, RT2, F2, K2)
    # (a) without neighbours: tray_denoise_demodulated_device with radius2 >= 1
    got = two_pass_guarded(frames[:1], r, rt, f, K, *second)
    want = FH.demodulated_guarded(*frames[0], r, f, K, (R2, F2, K2))
    assert same_bits(got, want), ("a", differing(got, want))
    # (b) albedo films without a valid pixel: tray_denoise_temporal_two_pass_device
    pairs = X.pairs_of(frames)
    want = T2.two_pass_guarded(pairs, r, rt, f, K, *second)
    for kind in ("zero-weight", "nan", "negative-weight"):
        got = two_pass_guarded([(e, o, TD.weightless_albedo(kind, w, h)) for e, o in pairs], r, rt, f, K, *second)
        assert same_bits(got, want), ("b", kind, differing(got, want))
    # (c) in general: numpy-f32 demodulation, tray_denoise_temporal_two_pass_device, numpy-f32 remodulation
    got = two_pass_guarded(frames, r, rt, f, K, *second)
    want_c = X.composed(lambda quotients: T2.two_pass_guarded(quotients, r, rt, f, K, *second), frames)
    assert same_bits(got, want_c), ("c", differing(got, want_c))
    assert not same_bits(got, want)
    # (d) this library's halves -- the centre's over all frames, every neighbour's alone -- followed by its guided call
    want_d = X.composition_of_own_calls(halves_guarded, guided_guarded, frames, r, rt, f, K, *second)
    assert same_bits(got, want_d), ("d", differing(got, want_d))


def test_python_gives_the_c_calls_bits(built):
    import torch
    w, h, (r, rt, f) = 33, 17, (7, 3, 3)
    frames = TD.random_frames(w, h, 3, seed=4)
    guides = X.random_guides(w, h, 3, seed=4)
    want = two_pass_guarded(frames, r, rt, f, K, R2, RT2, F2, K2)
    want_h = halves_guarded(frames, r, rt, f, K)
    want_g = guided_guarded(frames, guides, R2, RT2, F2, K2)
    hip = T.Hip(0)
    order = lambda x: [x[1], x[0], x[2]]   # the centre in the middle, the neighbours in list order
    fr, alb = [t[:2] for t in order(frames)], [t[2] for t in order(frames)]
    got = hip.denoise_temporal_demodulated(fr, alb, 1, r, rt, f, K)   # passes=2 and (5, 3, 1, 1.0) are the defaults
    assert isinstance(got, np.ndarray) and same_bits(got, want)
    assert same_bits(hip.denoise_temporal_demodulated(fr, alb, 1, r, rt, f, K, passes=1), hip.denoise_temporal(fr, 1, r, rt, f, K, albedos=alb))
    got_h = hip.denoise_temporal_demodulated_halves(fr, alb, 1, r, rt, f, K)
    assert all(isinstance(x, np.ndarray) and same_bits(x, y) for x, y in zip(got_h, want_h))
    assert same_bits(hip.denoise_temporal_demodulated_guided(fr, alb, order(guides), 1), want_g)
    up = lambda prs: [tuple(torch.from_numpy(x).cuda() for x in pr) for pr in prs]
    dev, adev, gdev = up(fr), [torch.from_numpy(a).cuda() for a in alb], up(order(guides))
    t = hip.denoise_temporal_demodulated(dev, adev, 1, r, rt, f, K)
    assert isinstance(t, torch.Tensor) and t.is_cuda and same_bits(t.cpu().numpy(), want)
    th = hip.denoise_temporal_demodulated_halves(dev, adev, 1, r, rt, f, K)
    assert all(isinstance(x, torch.Tensor) and same_bits(x.cpu().numpy(), y) for x, y in zip(th, want_h))
    assert same_bits(hip.denoise_temporal_demodulated_guided(dev, adev, gdev, 1).cpu().numpy(), want_g)
    one = hip.denoise_temporal_demodulated([frames[0][:2]], [frames[0][2]], 0, r, rt, f, K)
    assert same_bits(one, hip.denoise(*frames[0][:2], r, f, K, passes=2, albedo=frames[0][2]))


W, H, SPP = 48, 32, 8


def test_a_rendered_textured_sequence(tmp_path):
    """textured_box over three frames at 48 x 32, 8 spp, reach 1: every frame render_sequence_demodulated yields equals
    denoise_temporal_demodulated(passes=2) of films rendered separately with the same ranges and seed, the equality the existing sequence tests
    assert -- of the very films it rendered, read at the filter's call: a film is a sum of float atomics, so a second render need not give the
    same bits --; every albedo film is rendered once and every frame's own halves are computed once."""
    import torch
    scene, rt_, _, fi = TD.textured_sequence(str(tmp_path), W, H, SPP)
    cfg = T.Config(str(tmp_path), "textured_box.json", SPP, 1, fi)
    hip = T.Hip(0, seed=9)
    albedo_renders, pilots = [], []
    first_hit, halves = hip.render_first_hit_device, hip._denoise_temporal_demodulated_halves_device

    def first_hit_spy(scene_, frame, select_blocks, spp, rng, *a, **kw):
        albedo_renders.append((int(frame), tuple(int(v) for v in rng), int(spp)))
        return first_hit(scene_, frame, select_blocks, spp, rng, *a, **kw)

    def halves_spy(centre, neighbours, *a):
        torch.cuda.synchronize()
        pilots.append([tuple(x.cpu().numpy() for x in fr) for fr in [centre] + list(neighbours)])
        return halves(centre, neighbours, *a)

    hip.render_first_hit_device, hip._denoise_temporal_demodulated_halves_device = first_hit_spy, halves_spy
    got = list(hip.render_sequence_demodulated(scene, cfg, range(3), reach=1))
    assert [f for f, _ in got] == [0, 1, 2]
    assert sorted(albedo_renders) == [(g, (0, SPP), SPP) for g in range(3)], albedo_renders   # each once
    # a frame's own halves when it is rendered (no neighbours), the centre's over its window when it is filtered
    assert [len(p) for p in pilots] == [1, 1, 2, 1, 3, 2], [len(p) for p in pilots]
    own = [p[0][0].tobytes() for p in pilots if len(p) == 1]
    assert len(own) == 3 and len(set(own)) == 3   # each frame's once
    other = T.Hip(0, seed=9)
    for (f, img), frames in zip(got, [p for p in pilots if len(p) > 1]):
        want = other.denoise_temporal_demodulated([fr[:2] for fr in frames], [fr[2] for fr in frames], 0)
        assert img.shape == (H, W, 4) and same_bits(img, want), (f, differing(img, want))
    X.assert_two_pass(got[1][1], pilots[4], 7, 3, 3, K, R2, RT2, F2, K2, "render_sequence_demodulated, frame 1")
    scene.release_device()
