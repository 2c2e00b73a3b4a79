"""The kernels of tray_denoise_temporal_demodulated_halves_device, tray_denoise_temporal_demodulated_guided_device and
tray_denoise_temporal_demodulated_two_pass_device (k_tdm_prepare and k_td2_guided_pass of td2pass_kernels.h between the unchanged k_dn_prepare,
k_t2p_halves_pass and k_dn_filter_halves) in the host emulation (tests/emu/emu_td2pass.cpp), against the three calls' numpy statements
(tests/_td2pass_ref.py: every frame divided by the scale of its own albedo film, the two-pass temporal statements of the quotients, times the
centre's scale).

The bar is _td2pass_ref's: 4 x what the f32 statement differs from the f64 one, plus 1e-7, times the largest s_0, over the whole image and over
the centre's valid pixels. Then the identities of include/trayhip.h to the bit: (a) without neighbours the two-pass call is
tray_denoise_demodulated_device with radius2 >= 1; (b) with albedo films without a valid pixel it is tray_denoise_temporal_two_pass_device;
(c) in general it is numpy-f32 demodulation, the emulated two-pass temporal call, numpy-f32 remodulation; (d) it is this library's halves call
(the centre's over all frames, every neighbour's alone) followed by its guided call. That the albedo is each frame's own, and that it denoises
a textured sequence better than either pair of options: three frames of the oracle's textured_box."""
import json
import os

import numpy as np
import pytest

import tray_rust_amd as T
from tray_rust_amd import scenes
import _first_hit_ref as FH
import _oracle as O
import _ranges
import _td2pass_ref as X
import _tdemod_ref as TD
import _temporal_ref as TR
import _temporal2_ref as T2
from _denoise_ref import rgb, rmse

F32 = np.float32
K = 0.45


@pytest.fixture(scope="module")
def emu():
    return X.td2pass_lib()


SIZES = [(5, 3), (20, 12), (67, 45)]   # smaller than a window; not multiples of the 32 x 16 tile; more than one tile
RTF = [(1, 1, 0), (7, 3, 3), (10, 7, 3)]   # tests/test_tdemod_emu.py's
SECOND = [(1, 1, 0, 1.0), (5, 3, 1, 1.0)]
NS = [0, 2, 8]
IDS = [f"r{r}t{rt}f{f}" for r, rt, f in RTF]
IDS2 = [f"second{r}t{rt}f{f}" for r, rt, f, _ in SECOND]
SIZE_IDS = [f"{w}x{h}" for w, h in SIZES]


def seed_of(w, h):
    return 11 * w + h


def differing(a, b):
    return int((np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32)).sum())


# ---- under the bars, between guard words, the films unchanged

@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("r,rt,f", RTF, ids=IDS)
@pytest.mark.parametrize("w,h", SIZES, ids=SIZE_IDS)
def test_emulated_halves_match_the_f64_statement(emu, w, h, r, rt, f, n):
    frames = TD.random_frames(w, h, n + 1, seed=seed_of(w, h))
    fa, fb = X.run_halves(emu, frames, r, rt, f, K)
    X.assert_halves(fa, fb, frames, r, rt, f, K, f"halves {w}x{h} r={r} rt={rt} f={f} N={n}")


@pytest.mark.parametrize("r,rt,f,k", SECOND, ids=IDS2)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("w,h", SIZES, ids=SIZE_IDS)
def test_emulated_guided_call_matches_the_f64_statement(emu, w, h, n, r, rt, f, k):
    """guides that are no films of the frames, at the second pass's parameters"""
    frames = TD.random_frames(w, h, n + 1, seed=seed_of(w, h))
    guides = X.random_guides(w, h, n + 1, seed=seed_of(w, h))
    out = X.run_guided(emu, frames, guides, r, rt, f, k)
    X.assert_guided(out, frames, guides, r, rt, f, k, f"guided {w}x{h} r={r} rt={rt} f={f} N={n}")


@pytest.mark.parametrize("r2,rt2,f2,k2", SECOND, ids=IDS2)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("r,rt,f", RTF, ids=IDS)
@pytest.mark.parametrize("w,h", SIZES, ids=SIZE_IDS)
def test_emulated_two_pass_call_matches_the_f64_statement(emu, w, h, r, rt, f, n, r2, rt2, f2, k2):
    seed = seed_of(w, h)
    frames = TD.random_frames(w, h, n + 1, seed=seed)
    out = X.run_two_pass(emu, frames, r, rt, f, K, r2, rt2, f2, k2)
    X.assert_two_pass(out, frames, r, rt, f, K, r2, rt2, f2, k2, f"two-pass {w}x{h} r={r} rt={rt} f={f} N={n} second=({r2}, {rt2}, {f2})",
                      random_key=(w, h, n, seed))


# ---- the identities, to the bit

@pytest.mark.parametrize("r2,rt2,f2,k2", SECOND, ids=IDS2)
@pytest.mark.parametrize("r,rt,f", RTF, ids=IDS)
def test_without_neighbours_it_is_the_demodulated_two_pass_call(emu, r, rt, f, r2, rt2, f2, k2):
    """identity (a); it also holds tdm_scale and fh_scale together on albedo films with invalid, zero and negative pixels"""
    for w, h in SIZES:
        (even, odd, albedo), = TD.random_frames(w, h, 1, seed=7 * w + h)
        want = FH.emu_demodulated(even, odd, albedo, r, f, K, (r2, f2, k2))
        got = X.run_two_pass(emu, [(even, odd, albedo)], r, rt, f, K, r2, rt2, f2, k2)
        assert X.same_bits(got, want), (w, h, differing(got, want))


@pytest.mark.parametrize("kind", ["zero-weight", "nan", "negative-weight"])
def test_albedo_films_without_weight_give_the_two_pass_temporal_calls_bits(emu, kind):
    """identity (b)"""
    t2 = T2.temporal2_lib()
    for (w, h), (r, rt, f), n in [((20, 12), (7, 3, 3), 2), ((67, 45), (3, 2, 1), 3), ((41, 23), (10, 7, 3), 1)]:
        pairs = TR.random_frames(w, h, n + 1, seed=3 + w)
        dead = TD.weightless_albedo(kind, w, h) if kind != "negative-weight" else -np.abs(FH.random_albedo(w, h, 3))
        got = X.run_two_pass(emu, [(e, o, dead.copy()) for e, o in pairs], r, rt, f, K, *X.DEFAULTS2)
        assert X.same_bits(got, T2.run_two_pass(t2, pairs, r, rt, f, K, *X.DEFAULTS2)), (w, h, kind)


@pytest.mark.parametrize("r2,rt2,f2,k2", SECOND, ids=IDS2)
@pytest.mark.parametrize("n", [1, 2, 8])
@pytest.mark.parametrize("r,rt,f", RTF, ids=IDS)
def test_it_is_the_composition_of_the_three_steps(emu, r, rt, f, n, r2, rt2, f2, k2):
    """identity (c): numpy-f32 demodulation, the emulated tray_denoise_temporal_two_pass_device, numpy-f32 remodulation"""
    t2 = T2.temporal2_lib()
    for w, h in [(20, 12), (67, 45)][:1 if n == 8 else 2]:
        frames = TD.random_frames(w, h, n + 1, seed=5 * w + h + n)
        want = X.composed(lambda pairs: T2.run_two_pass(t2, pairs, r, rt, f, K, r2, rt2, f2, k2), frames)
        got = X.run_two_pass(emu, frames, r, rt, f, K, r2, rt2, f2, k2)
        assert X.same_bits(got, want), (w, h, differing(got, want))


@pytest.mark.parametrize("r2,rt2,f2,k2", SECOND, ids=IDS2)
@pytest.mark.parametrize("n", [1, 2, 8])
@pytest.mark.parametrize("r,rt,f", RTF, ids=IDS)
def test_it_is_its_own_halves_followed_by_its_guided_call(emu, r, rt, f, n, r2, rt2, f2, k2):
    """identity (d); the halves and the guided call against the undemodulated calls on the numpy-f32 quotients on the way: the halves to the
    bit, the guided call up to the remodulation (identity (c)'s form)"""
    t2 = T2.temporal2_lib()
    for w, h in [(20, 12), (67, 45)][:1 if n == 8 else 2]:
        frames = TD.random_frames(w, h, n + 1, seed=5 * w + h + n)
        got = X.run_two_pass(emu, frames, r, rt, f, K, r2, rt2, f2, k2)
        halves = lambda fr, *a: X.run_halves(emu, fr, *a)
        guided = lambda fr, g, *a: X.run_guided(emu, fr, g, *a)
        want = X.composition_of_own_calls(halves, guided, frames, r, rt, f, K, r2, rt2, f2, k2)
        assert X.same_bits(got, want), (w, h, differing(got, want))
        own = X.run_halves(emu, frames, r, rt, f, K)
        plain = T2.run_halves(t2, X.demodulated_pairs(frames), r, rt, f, K)
        assert all(X.same_bits(a, b) for a, b in zip(own, plain)), (w, h, "halves")
        guides = X.random_guides(w, h, n + 1, seed=w)
        g_own = X.run_guided(emu, frames, guides, r2, rt2, f2, k2)
        g_plain = X.composed(lambda pairs: T2.run_guided(t2, pairs, guides, r2, rt2, f2, k2), frames)
        assert X.same_bits(g_own, g_plain), (w, h, "guided", differing(g_own, g_plain))


def test_scratch_bytes(emu):
    for name, per_pixel in (("halves", 128), ("guided", 176), ("two_pass", 256)):
        fn = getattr(emu, f"emu_td2_{name}_scratch_bytes")
        assert fn(0, 5) == 0 and fn(5, 0) == 0 and fn(67, 45) == 67 * 45 * per_pixel and fn(65535, 65535) == 65535 * 65535 * per_pixel
        assert fn(67, 45) == getattr(T2.temporal2_lib(), f"emu_temporal_{name}_scratch_bytes")(67, 45)   # the two-pass temporal call's


def test_every_frame_is_divided_by_its_own_albedo(emu):
    w, h, (r, rt, f) = 41, 23, (7, 3, 3)
    frames = TD.random_frames(w, h, 3, seed=2)
    out = X.run_two_pass(emu, frames, r, rt, f, K, *X.DEFAULTS2)
    (e1, o1, a1), (e2, o2, a2) = frames[1:]
    swapped_frames = [frames[0], (e1, o1, a2), (e2, o2, a1)]
    swapped = X.run_two_pass(emu, swapped_frames, r, rt, f, K, *X.DEFAULTS2)
    assert not X.same_bits(out, swapped)
    X.assert_two_pass(swapped, swapped_frames, r, rt, f, K, *X.DEFAULTS2, "neighbours' albedo films swapped")
    halves, swapped_halves = X.run_halves(emu, frames, r, rt, f, K), X.run_halves(emu, swapped_frames, r, rt, f, K)
    assert not X.same_bits(halves[0], swapped_halves[0])


# ---- it is better where the texture changes from frame to frame: films of the oracle (tests/test_tdemod_emu.py's)

W = H = 64
SPP, SPLIT, REF_SPP, SEED, REF_SEED = 32, 16, 1024, 7, 1234
R_, RT_, F_ = 7, 3, 3


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
    ref = rgb(O.render_tiles(scene.flatten(centre), REF_SPP, seed=REF_SEED)[0])
    even, odd, _ = frames[0]
    temporal = TR.run(TR.temporal_lib(), X.pairs_of(frames), R_, RT_, F_, K)
    tdemod = TD.run(TD.tdemod_lib(), frames, R_, RT_, F_, K)
    t2pass = T2.run_two_pass(T2.temporal2_lib(), X.pairs_of(frames), R_, RT_, F_, K, *X.DEFAULTS2)
    all_three = X.run_two_pass(emu, frames, R_, RT_, F_, K, *X.DEFAULTS2)
    X.assert_two_pass(all_three, frames, R_, RT_, F_, K, *X.DEFAULTS2, f"{what} oracle films")
    e = [rmse(x, ref) for x in (rgb(even + odd), temporal[..., :3], tdemod[..., :3], t2pass[..., :3], all_three[..., :3])]
    print(f"{what} {W}x{H} {SPP} spp, frames {centre - 1} - {centre + 1}: RMSE(noisy) = {e[0]:.6f}, RMSE(temporal) = {e[1]:.6f}, "
          f"RMSE(temporal + demodulated) = {e[2]:.6f}, RMSE(two-pass temporal) = {e[3]:.6f}, RMSE(two-pass temporal + demodulated) = {e[4]:.6f}: "
          f"{e[4] / min(e[2], e[3]):.3f} x the better of the two")
    return e


def test_it_denoises_a_textured_sequence_better_than_either_pair_of_options(emu, tmp_path, built):
    """textured_box over three frames (scene_time 1, shutter 0.5), frame 1 with frames 0 and 2 at 32 spp, against 1024 spp of frame 1 of another
    seed: 0.008598 against 0.009494 (temporal + demodulated) and 0.010155 (two-pass temporal)"""
    scene = TD.textured_sequence(str(tmp_path), W, H, SPP)[0]
    noisy, temporal, tdemod, t2pass, all_three = five_numbers(emu, scene, 1, "textured_box")
    assert all_three < min(tdemod, t2pass)


def test_moving_box_row_is_printed(emu, tmp_path, built):
    """printed only: moving_box has no texture, so about 1.0 x the two-pass temporal call is expected"""
    scenes.write_assets(str(tmp_path))
    p = os.path.join(str(tmp_path), "s.json")
    with open(p, "w") as fh:
        json.dump(scenes.moving_box(W, H, SPP, frames=48), fh)
    five_numbers(emu, T.Scene.load_file(p)[0], 24, "moving_box")
