"""tray_denoise_temporal_demodulated_device's kernels (k_tdm_prepare, k_dn_prepare<1>, k_tdm_pass of tdemod_kernels.h) in the host emulation
(tests/emu/emu_tdemod.cpp), against the call's numpy statement (tests/_tdemod_ref.py: every frame divided by the scale of its own albedo film,
_temporal_ref.temporal of the quotients, times the centre's scale).

The bar is _tdemod_ref.bar: the temporal bar -- 4 x what the f32 statement differs from the f64 one, plus 1e-7 -- times the largest s_0, and the
same rule over the centre's valid pixels. Then the three identities of include/trayhip.h to the bit: (a) without neighbours the call is
tray_denoise_demodulated_device, which also holds tdm_scale and fh_scale together on albedo films with invalid, zero and negative pixels;
(b) with albedo films without a valid pixel it is tray_denoise_temporal_device; (c) in general it is numpy-f32 demodulation, the emulated
temporal call, numpy-f32 remodulation. That the albedo is each frame's own, and that it denoises a textured sequence better than either
existing call: three frames of the oracle's textured_box, whose blink wall and film strip change from frame to frame."""
import json
import os

import numpy as np
import pytest

import tray_rust_amd as T
from tray_rust_amd import scenes
import _emu_features as EF
import _first_hit_ref as FH
import _oracle as O
import _ranges
import _tdemod_ref as TD
import _temporal_ref as TR
from _denoise_ref import rgb, rmse

F32 = np.float32


@pytest.fixture(scope="module")
def emu():
    return TD.tdemod_lib()


SIZES = [(5, 3), (20, 12), (67, 45)]   # smaller than a window; not multiples of the 32 x 16 tile
RTF = [(1, 1, 0), (7, 3, 3), (10, 7, 3)]
IDS = [f"r{r}t{rt}f{f}" for r, rt, f in RTF]


@pytest.mark.parametrize("n", [0, 2, 8])
@pytest.mark.parametrize("r,rt,f", RTF, ids=IDS)
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_emulated_kernels_match_the_f64_statement(emu, w, h, r, rt, f, n):
    frames = TD.random_frames(w, h, n + 1, seed=11 * w + h)
    for even, odd, albedo in frames:
        valid = (albedo[..., 3] > 0) & np.isfinite(albedo).all(-1)
        assert (~valid).any()
        assert (w, h) == (5, 3) or ((albedo[valid][:, :3] == 0).any() and (albedo[valid][:, :3] < 0).any())   # (15 pixels: the few picks may coincide)
    out = TD.run(emu, frames, r, rt, f, 0.45)   # (between guard words, the films unchanged)
    TD.assert_matches(out, frames, r, rt, f, 0.45, f"{w}x{h} r={r} rt={rt} f={f} N={n}")


@pytest.mark.parametrize("r,rt,f", RTF, ids=IDS)
def test_without_neighbours_it_is_the_demodulated_call(emu, r, rt, f):
    """identity (a)"""
    for w, h in SIZES:
        (even, odd, albedo), = TD.random_frames(w, h, 1, seed=7 * w + h)
        want = FH.emu_demodulated(even, odd, albedo, r, f, 0.45)
        got = TD.run(emu, [(even, odd, albedo)], r, rt, f, 0.45)
        assert TD.same_bits(got, want), (w, h, int((got.view(np.uint32) != want.view(np.uint32)).sum()))


@pytest.mark.parametrize("kind", ["zero-weight", "nan", "negative-weight"])
def test_albedo_films_without_weight_give_the_temporal_calls_bits(emu, kind):
    """identity (b)"""
    temporal = TR.temporal_lib()
    for (w, h), (r, rt, f), n in [((20, 12), (7, 3, 3), 2), ((67, 45), (3, 2, 1), 3), ((41, 23), (10, 7, 3), 1)]:
        pairs = TR.random_frames(w, h, n + 1, seed=3 + w)
        dead = TD.weightless_albedo(kind, w, h) if kind != "negative-weight" else -np.abs(FH.random_albedo(w, h, 3))
        got = TD.run(emu, [(e, o, dead.copy()) for e, o in pairs], r, rt, f, 0.45)
        assert TD.same_bits(got, TR.run(temporal, pairs, r, rt, f, 0.45)), (w, h, kind)


@pytest.mark.parametrize("n", [1, 2, 8])
@pytest.mark.parametrize("r,rt,f", RTF, ids=IDS)
def test_it_is_the_composition_of_the_three_steps(emu, r, rt, f, n):
    """identity (c): numpy-f32 demodulation, the emulated tray_denoise_temporal_device, numpy-f32 remodulation"""
    temporal = TR.temporal_lib()
    for w, h in [(20, 12), (67, 45)][:1 if n == 8 else 2]:
        frames = TD.random_frames(w, h, n + 1, seed=5 * w + h + n)
        want = TD.composed(lambda pairs: TR.run(temporal, pairs, r, rt, f, 0.45), frames)
        got = TD.run(emu, frames, r, rt, f, 0.45)
        assert TD.same_bits(got, want), (w, h, int((got.view(np.uint32) != want.view(np.uint32)).sum()))


def test_scratch_bytes(emu):
    assert emu.emu_tdemod_scratch_bytes(0, 5) == 0 and emu.emu_tdemod_scratch_bytes(5, 0) == 0
    assert emu.emu_tdemod_scratch_bytes(67, 45) == 67 * 45 * 128 == TR.temporal_lib().emu_temporal_scratch_bytes(67, 45)


def test_every_frame_is_divided_by_its_own_albedo(emu):
    w, h, (r, rt, f) = 41, 23, (7, 3, 3)
    frames = TD.random_frames(w, h, 3, seed=2)
    out = TD.run(emu, frames, r, rt, f, 0.45)
    (e1, o1, a1), (e2, o2, a2) = frames[1:]
    swapped = TD.run(emu, [frames[0], (e1, o1, a2), (e2, o2, a1)], r, rt, f, 0.45)
    assert not TD.same_bits(out, swapped)
    TD.assert_matches(swapped, [frames[0], (e1, o1, a2), (e2, o2, a1)], r, rt, f, 0.45, "neighbours' albedo films swapped")


def test_albedo_equal_to_the_colour_leaves_a_near_constant_image(emu):
    """albedo = E + O in every frame: the quotients are a(p) / (a(p) + eps) with a the resolved colour, in [0.9375, 1] for a colour in
    [0.15, 0.95]: the demodulated films are near-constant whatever the colour does. Every output channel is the centre's own s_0 times a mean
    of quotients of its windows, so it lies within that spread of the centre's own colour -- whatever the neighbours' colours are. (The two
    halves carry no noise here, so V is 0 and only equal patches weigh: the output is the pixel's own colour almost to the bit.)"""
    rng = np.random.default_rng(8)
    w, h = 40, 24
    frames = []
    for j in range(3):
        yy, xx = np.mgrid[0:h, 0:w]
        colour = np.stack([0.55 + 0.4 * np.sin(xx * (0.7 + 0.2 * j) + c) * np.cos(yy * 0.5 - c - j) for c in range(3)], -1)   # in [0.15, 0.95]
        pair = []
        for _ in range(2):
            wgt = rng.uniform(0.5, 8.0, (h, w, 1))
            pair.append(np.concatenate([colour * wgt, wgt], -1).astype(F32))
        frames.append((pair[0], pair[1], (pair[0] + pair[1]).astype(F32)))
    quotients = TD.demodulated_frames(frames, F32)
    for e, o in quotients:
        a = e[..., :3] / e[..., 3:]
        assert a.min() >= 0.15 / 0.16 - 1e-3 and a.max() <= 1.0   # near-constant: in [0.9375, 1]
    out = TD.run(emu, frames, 7, 3, 3, 0.45)
    TD.assert_matches(out, frames, 7, 3, 3, 0.45, "albedo = E + O")
    own = rgb(frames[0][2])
    rel = np.abs(out[..., :3] - own) / own
    print(f"albedo = E + O: the output differs from the centre's own colour by at most {rel.max():.4f} relative")
    assert rel.max() <= 1.0 / 0.9375 - 1.0 + 1e-3   # the quotients' spread


# ---- it is better where the texture changes from frame to frame: films of the oracle

W = H = 64
SPP, SPLIT, REF_SPP, SEED, REF_SEED = 32, 16, 1024, 7, 1234
R_, RT_, F_, K_ = 7, 3, 3, 0.45


def oracle_frames(scene, frame_numbers):
    """frame -> (even, odd, albedo): the oracle's range films of [0, 16) and [16, 32), the albedo film of [0, 32) from the per-sample statement"""
    q = _ranges.tile_queue(W, H)
    items = FH.frame_items(q, SPP)
    out = {}
    for g in frame_numbers:
        flat = scene.flatten(g)
        even, odd = (_ranges.oracle_range(flat, q, rng, SPP, SEED)[0] for rng in ((0, SPLIT), (SPLIT, SPP)))
        albedo = FH.films_of(flat, q, items, FH.records(flat, *items[:3], SPP, SEED), (0, SPP), which=(0,))[0]
        out[g] = (even, odd, albedo)
    return out


def five_numbers(emu, scene, centre, what):
    fr = oracle_frames(scene, (centre - 1, centre, centre + 1))
    frames = [fr[centre], fr[centre - 1], fr[centre + 1]]   # the neighbours in ascending frame order
    for g in (centre - 1, centre + 1):
        print(f"{what}: resolved albedo of frame {g} differs from frame {centre}'s by RMSE {rmse(rgb(fr[g][2]), rgb(fr[centre][2])):.3f}")
    ref = rgb(O.render_tiles(scene.flatten(centre), REF_SPP, seed=REF_SEED)[0])
    even, odd, albedo = frames[0]
    plain = EF.denoise(EF.denoise_lib(), even, odd, R_, F_, K_)
    demod = FH.emu_demodulated(even, odd, albedo, R_, F_, K_)
    temporal = TR.run(TR.temporal_lib(), [fr_[:2] for fr_ in frames], R_, RT_, F_, K_)
    both = TD.run(emu, frames, R_, RT_, F_, K_)
    TD.assert_matches(both, frames, R_, RT_, F_, K_, f"{what} oracle films")
    e = [rmse(x, ref) for x in (rgb(even + odd), plain[..., :3], demod[..., :3], temporal[..., :3], both[..., :3])]
    print(f"{what} {W}x{H} {SPP} spp, frames {centre - 1} - {centre + 1}: RMSE(noisy) = {e[0]:.5f}, RMSE(plain) = {e[1]:.5f}, RMSE(demodulated) = {e[2]:.5f}, "
          f"RMSE(temporal) = {e[3]:.5f}, RMSE(temporal + demodulated) = {e[4]:.5f}: {e[4] / min(e[2], e[3]):.3f} x the better of the two, "
          f"{e[4] / e[1]:.3f} x the plain filter")
    return e


def test_it_denoises_a_textured_sequence_better_than_either_call(emu, tmp_path, built):
    """textured_box over three frames (scene_time 1, shutter 0.5), frame 1 with frames 0 and 2, against 1024 spp of frame 1"""
    scene = TD.textured_sequence(str(tmp_path), W, H, SPP)[0]
    noisy, plain, demod, temporal, both = five_numbers(emu, scene, 1, "textured_box")
    assert both < min(demod, temporal) < plain < noisy


def test_an_untextured_sequence_neither_gains_nor_loses(emu, tmp_path, built):
    """printed only: moving_box has no texture, so about 1.0 x the temporal call is expected"""
    scenes.write_assets(str(tmp_path))
    p = os.path.join(str(tmp_path), "s.json")
    with open(p, "w") as fh:
        json.dump(scenes.moving_box(W, H, SPP, frames=48), fh)
    five_numbers(emu, T.Scene.load_file(p)[0], 24, "moving_box")
