"""The kernels of tray_denoise_temporal_halves_device, tray_denoise_temporal_guided_device and tray_denoise_temporal_two_pass_device
(k_t2p_halves_pass, k_t2p_guided_pass of t2pass_kernels.h between the unchanged k_dn_prepare and k_dn_filter_halves) in the host emulation
(tests/emu/emu_temporal2.cpp), against the three calls' numpy statements (tests/_temporal2_ref.py).

The bar is _guided_ref.bar_of: 4 x what the f32 statement differs from the f64 one, plus 1e-7, over the whole image and over the centre's valid
pixels. Then the identities of include/trayhip.h to the bit against the emulated existing calls -- the halves' mean is the temporal call, the
halves without neighbours are tray_denoise_halves_device, the guided call with the frames as their own guides is the temporal call, the guided
call without neighbours is tray_denoise_guided_device, the two-pass call without neighbours is tray_denoise_two_pass_device --, the two-pass call
against its composition, that every frame's guide is its own, the range property over all windows, and that it denoises: three frames of the
oracle's textured_box, where the new call must beat both the temporal call and the two-pass call of the centre frame alone."""
import json
import os

import numpy as np
import pytest

import tray_rust_amd as T
from tray_rust_amd import scenes
import _emu_features as EF
import _guided_ref as G
import _oracle as O
import _ranges
import _tdemod_ref as TD
import _temporal_ref as TR
import _temporal2_ref as T2
from _denoise_ref import rgb, rmse, resolve

F32, F64 = np.float32, np.float64
K = 0.45


@pytest.fixture(scope="module")
def emu():
    return T2.temporal2_lib()


SIZES = [(5, 3), (20, 12), (67, 45)]   # smaller than a window; not multiples of the 32 x 16 tile; more than one tile
RTF = [(1, 1, 0), (7, 3, 3), (10, 7, 3)]
SECOND = [(5, 3, 1, 1.0), (3, 2, 0, 1.0)]
NS = [0, 2, 8]
IDS = [f"r{r}t{rt}f{f}" for r, rt, f in RTF]
IDS2 = [f"second{r}t{rt}f{f}" for r, rt, f, _ in SECOND]
SIZE_IDS = [f"{w}x{h}" for w, h in SIZES]


def seed_of(w, h):
    return 11 * w + h


# ---- the statements hold together (numpy only)

def test_the_statement_is_the_temporal_and_the_guided_statement_where_they_apply():
    """f32 values, exactly: with the frames as their own guides the mean of halves() is _temporal_ref.temporal; with one frame halves() is
    _guided_ref.halves"""
    frames = TR.random_frames(20, 12, 3, seed=4)
    guides = T2.random_guides(20, 12, 3, seed=4)
    A, B, _, _ = T2.halves(frames, frames, 3, 2, 1, K, F32)
    assert T2.same_bits(((A + B) * F32(0.5)).astype(F32), TR.temporal(frames, 3, 2, 1, K, F32))
    one = T2.halves(frames[:1], guides[:1], 3, 2, 1, K, F32)
    ref = G.halves(*frames[0], *guides[0], 3, 1, K, F32)
    assert all(T2.same_bits(x.astype(F32), y.astype(F32)) for x, y in zip(one, ref))


# ---- under the bars, between guard words, the films unchanged

@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("r,rt,f", RTF, ids=IDS)
@pytest.mark.parametrize("w,h", SIZES, ids=SIZE_IDS)
def test_emulated_halves_match_the_f64_statement(emu, w, h, r, rt, f, n):
    frames = TR.random_frames(w, h, n + 1, seed=seed_of(w, h))
    fa, fb = T2.run_halves(emu, frames, r, rt, f, K)
    T2.assert_halves(fa, fb, frames, r, rt, f, K, f"halves {w}x{h} r={r} rt={rt} f={f} N={n}")


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("r,rt,f", RTF, ids=IDS)
@pytest.mark.parametrize("w,h", SIZES, ids=SIZE_IDS)
def test_emulated_guided_call_matches_the_f64_statement(emu, w, h, r, rt, f, n):
    """guides that are no films of the frames: their invalid pixels lie elsewhere, so pixels invalid in the values and valid in the guide (filled
    from their windows) and the other way round both occur"""
    frames = TR.random_frames(w, h, n + 1, seed=seed_of(w, h))
    guides = T2.random_guides(w, h, n + 1, seed=seed_of(w, h))
    v, g = resolve(*frames[0])[0], resolve(*guides[0])[0]
    assert (v & ~g).any() or (w, h) == (5, 3)
    out = T2.run_guided(emu, frames, guides, r, rt, f, 1.0)
    T2.assert_guided(out, frames, guides, r, rt, f, 1.0, f"guided {w}x{h} r={r} rt={rt} f={f} N={n}")


@pytest.mark.parametrize("r2,rt2,f2,k2", SECOND, ids=IDS2)
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("r,rt,f", RTF, ids=IDS)
@pytest.mark.parametrize("w,h", SIZES, ids=SIZE_IDS)
def test_emulated_two_pass_call_matches_the_f64_statement(emu, w, h, r, rt, f, n, r2, rt2, f2, k2):
    seed = seed_of(w, h)
    frames = TR.random_frames(w, h, n + 1, seed=seed)
    out = T2.run_two_pass(emu, frames, r, rt, f, K, r2, rt2, f2, k2)
    T2.assert_two_pass(out, frames, r, rt, f, K, r2, rt2, f2, k2, f"two-pass {w}x{h} r={r} rt={rt} f={f} N={n} second=({r2}, {rt2}, {f2})",
                       random_key=(w, h, n, seed))


# ---- the identities, to the bit, against the emulated existing calls

def differing(a, b):
    return int((np.asarray(a).view(np.uint32) != np.asarray(b).view(np.uint32)).sum())


@pytest.mark.parametrize("n", [1, 2, 8])
@pytest.mark.parametrize("r,rt,f", RTF, ids=IDS)
def test_the_halves_mean_is_the_temporal_call(emu, r, rt, f, n):
    for w, h in SIZES[:2 if n == 8 else 3]:
        frames = TR.random_frames(w, h, n + 1, seed=7 * w + h)
        fa, fb = T2.run_halves(emu, frames, r, rt, f, K)
        want = TR.run(TR.temporal_lib(), frames, r, rt, f, K)
        mean = ((fa[..., :3] + fb[..., :3]) * F32(0.5)).astype(F32)
        assert T2.same_bits(mean, want[..., :3]), (w, h, differing(mean, want[..., :3]))


@pytest.mark.parametrize("r,rt,f", RTF, ids=IDS)
def test_halves_without_neighbours_are_the_single_frame_halves(emu, r, rt, f):
    for w, h in SIZES:
        frames = TR.random_frames(w, h, 1, seed=7 * w + h)
        got = T2.run_halves(emu, frames, r, rt, f, K)
        want = EF.guide_halves(EF.guide_lib(), *frames[0], r, f, K)
        assert all(T2.same_bits(x, y) for x, y in zip(got, want)), (w, h, [differing(x, y) for x, y in zip(got, want)])


@pytest.mark.parametrize("n", [1, 2, 8])
@pytest.mark.parametrize("r,rt,f", RTF, ids=IDS)
def test_guided_by_its_own_frames_it_is_the_temporal_call(emu, r, rt, f, n):
    """identity (i), the guide pointers being the films'"""
    for w, h in SIZES[:2 if n == 8 else 3]:
        frames = T2._contiguous(TR.random_frames(w, h, n + 1, seed=3 * w + h))
        got = T2.run_guided(emu, frames, frames, r, rt, f, K)
        want = TR.run(TR.temporal_lib(), frames, r, rt, f, K)
        assert T2.same_bits(got, want), (w, h, differing(got, want))


@pytest.mark.parametrize("r,rt,f", RTF, ids=IDS)
def test_guided_without_neighbours_it_is_the_guided_call(emu, r, rt, f):
    """identity (ii)"""
    for w, h in SIZES:
        frames = TR.random_frames(w, h, 1, seed=5 * w + h)
        guides = T2.random_guides(w, h, 1, seed=5 * w + h)
        got = T2.run_guided(emu, frames, guides, r, rt, f, 1.0)
        want = G.run_guided(G.guided_lib(), *frames[0], *guides[0], r, f, 1.0)
        assert T2.same_bits(got, want), (w, h, differing(got, want))


@pytest.mark.parametrize("r2,rt2,f2,k2", SECOND, ids=IDS2)
@pytest.mark.parametrize("r,rt,f", RTF, ids=IDS)
def test_two_pass_without_neighbours_is_the_single_frame_two_pass_call(emu, r, rt, f, r2, rt2, f2, k2):
    for w, h in SIZES:
        frames = TR.random_frames(w, h, 1, seed=9 * w + h)
        got = T2.run_two_pass(emu, frames, r, rt, f, K, r2, rt2, f2, k2)
        want = G.run_two_pass(G.guided_lib(), *frames[0], r, f, K, r2, f2, k2)
        assert T2.same_bits(got, want), (w, h, differing(got, want))


@pytest.mark.parametrize("r2,rt2,f2,k2", SECOND, ids=IDS2)
@pytest.mark.parametrize("n", [1, 2, 8])
@pytest.mark.parametrize("r,rt,f", RTF, ids=IDS)
def test_the_two_pass_call_is_its_composition(emu, r, rt, f, n, r2, rt2, f2, k2):
    """the temporal halves of the centre, tray_denoise_halves_device of every neighbour, the guided call: each emulated on its own"""
    for w, h in [(20, 12), (67, 45)][:1 if n == 8 else 2]:
        frames = TR.random_frames(w, h, n + 1, seed=5 * w + h + n)
        got = T2.run_two_pass(emu, frames, r, rt, f, K, r2, rt2, f2, k2)
        want = T2.emulated_composition(emu, frames, r, rt, f, K, r2, rt2, f2, k2)
        assert T2.same_bits(got, want), (w, h, differing(got, want))


def test_scratch_bytes(emu):
    for name, per_pixel in (("halves", 128), ("guided", 176), ("two_pass", 256)):
        fn = getattr(emu, f"emu_temporal_{name}_scratch_bytes")
        assert fn(0, 5) == 0 and fn(5, 0) == 0 and fn(67, 45) == 67 * 45 * per_pixel and fn(65535, 65535) == 65535 * 65535 * per_pixel


# ---- every frame's guide is its own; the guides only choose weights

def test_swapping_two_neighbours_guides_changes_the_output(emu):
    w, h, (r, rt, f) = 41, 23, (5, 3, 1)
    frames = TR.random_frames(w, h, 3, seed=2)
    guides = T2.random_guides(w, h, 3, seed=2)
    out = T2.run_guided(emu, frames, guides, r, rt, f, 1.0)
    swapped = [guides[0], guides[2], guides[1]]
    other = T2.run_guided(emu, frames, swapped, r, rt, f, 1.0)
    assert not T2.same_bits(out, other)
    T2.assert_guided(other, frames, swapped, r, rt, f, 1.0, "neighbours' guides swapped")


@pytest.mark.parametrize("n", [0, 2])
def test_range_property_over_all_windows(emu, n):
    """every output channel lies within the VALUES' range over all frames' windows, whatever the guides hold: here guides of another image
    altogether (three times the values' level)"""
    w, h, (r, rt, f) = 67, 45, (5, 3, 1)
    frames = TR.random_frames(w, h, n + 1, seed=13)
    guides = [tuple((x * np.array([3, 3, 3, 1], F32)).astype(F32) for x in g) for g in T2.random_guides(w, h, n + 1, seed=13)]
    out = T2.run_guided(emu, frames, guides, r, rt, f, 1.0)
    assert len(T2.range_violations(out[..., :3], frames, r, rt, T2.sure_pixels(frames, guides))) == 0
    two = T2.run_two_pass(emu, frames, 7, 3, 3, K, r, rt, f, 1.0)
    assert len(T2.range_violations(two[..., :3], frames, r, rt, resolve(*frames[0])[0])) == 0


# ---- it denoises: films of the oracle

W = H = 64
SPP, SPLIT, REF_SPP, SEED, REF_SEED = 32, 16, 1024, 7, 1234
R_, RT_, F_ = 7, 3, 3
R2_, RT2_, F2_, K2_ = T2.DEFAULTS2


def oracle_frames(scene, frame_numbers, seed_of):
    """[(even, odd)] per frame number: the oracle's range films of [0, 16) and [16, 32); half film i of list entry j has the seed seed_of(j, i)"""
    q = _ranges.tile_queue(W, H)
    return [tuple(_ranges.oracle_range(scene.flatten(g), q, rng, SPP, seed_of(j, i))[0] for i, rng in enumerate(((0, SPLIT), (SPLIT, SPP))))
            for j, g in enumerate(frame_numbers)]


def five_numbers(emu, scene, centre, what, seed_of=lambda j, i: SEED, ref_spp=REF_SPP):
    frames = oracle_frames(scene, (centre, centre - 1, centre + 1), seed_of)   # the neighbours in ascending frame order
    ref = rgb(O.render_tiles(scene.flatten(centre), ref_spp, seed=REF_SEED)[0])
    even, odd = frames[0]
    plain = EF.denoise(EF.denoise_lib(), even, odd, R_, F_, K)
    alone = G.run_two_pass(G.guided_lib(), even, odd, R_, F_, K, R2_, F2_, K2_)
    temporal = TR.run(TR.temporal_lib(), frames, R_, RT_, F_, K)
    both = T2.run_two_pass(emu, frames, R_, RT_, F_, K, R2_, RT2_, F2_, K2_)
    e = [rmse(x, ref) for x in (rgb(even + odd), plain[..., :3], alone[..., :3], temporal[..., :3], both[..., :3])]
    print(f"{what} {W}x{H} {SPP} spp, frames {centre - 1} - {centre + 1}: RMSE(noisy) = {e[0]:.5f}, RMSE(plain) = {e[1]:.5f}, "
          f"RMSE(two-pass, one frame) = {e[2]:.5f}, RMSE(temporal) = {e[3]:.5f}, RMSE(two-pass temporal) = {e[4]:.5f}: "
          f"{e[4] / min(e[2], e[3]):.3f} x the better of the two, {e[4] / e[1]:.3f} x the plain filter")
    return e


def test_it_denoises_a_textured_sequence_better_than_either_call(emu, tmp_path, built):
    """textured_box over three frames (scene_time 1, shutter 0.5), frame 1 with frames 0 and 2, against 1024 spp of frame 1. The f64 statement
    gives 0.01015 against 0.01118 (two passes of frame 1 alone) and 0.01170 (temporal)."""
    scene = TD.textured_sequence(str(tmp_path), W, H, SPP)[0]
    noisy, plain, alone, temporal, both = five_numbers(emu, scene, 1, "textured_box")
    assert both < min(temporal, alone) < plain < noisy


def test_moving_box_row_is_printed(emu, tmp_path, built):
    """printed only: moving_box(frames=48), frames 23 - 25, every half film of a seed of its own and 2048 reference samples, as
    tests/test_temporal_emu.py has them"""
    scenes.write_assets(str(tmp_path))
    p = os.path.join(str(tmp_path), "s.json")
    with open(p, "w") as fh:
        json.dump(scenes.moving_box(W, H, SPP, frames=48), fh)
    five_numbers(emu, T.Scene.load_file(p)[0], 24, "moving_box", seed_of=lambda j, i: 7 + 10 * j + i, ref_spp=2048)
