"""tray_denoise_guided_device's and tray_denoise_two_pass_device's kernels (k_dn_prepare and k_dn_filter_halves of denoise_kernels.h / guide_kernels.h,
k_gdn_filter of guided_kernels.h) in the host emulation, against the numpy statements of the two calls (tests/_guided_ref.py, which restates
include/trayhip.h in float32 and float64).

tests/emu/emu_guided.cpp runs the launches of a call as SIMT fibers: the LDS staging of the guide, the two barriers per offset and the values'
loads execute as on the device. The bar of every comparison is _guided_ref.bar_of: the kernels may differ from the f64 statement by 4 x what
the f32 numpy statement differs from it on the same input, plus 1e-7. Then: the films as their own guide give tray_denoise_device's bits, the
two-pass call gives the bits of halves followed by guided, the range of the values, a constant colour, films and guides without a valid pixel,
a hole of the values filled through the guide, and that two passes denoise oracle films better than one: at 64 x 64 and 32 spp the f64
statement gives RMSE 0.00987 (two passes) / 0.01145 (one) / 0.01916 (noisy) on cornell_box and 0.01076 / 0.01252 / 0.02203 on smallpt against a
2048-spp oracle render of another seed."""
import json
import os

import numpy as np
import pytest

import tray_rust_amd as T
from tray_rust_amd import scenes
import _emu_features as EF
import _oracle as O
import _denoise_ref as D
import _ranges as R
import _guided_ref as G
from _denoise_ref import rgb, rmse

F32 = np.float32


@pytest.fixture(scope="module")
def emu():
    return G.guided_lib()


SIZES = [(5, 3), (20, 12), (67, 45)]   # smaller than a window; not multiples of the 32 x 16 tile
RF = [(1, 0), (3, 1), (7, 3), (10, 3)]   # test_denoise_emu.RF
bits = lambda x: np.ascontiguousarray(x).view(np.uint32)


def films_and_guide(w, h):
    """values and a guide of another seed: their invalid pixels differ"""
    return D.random_films(w, h, seed=11 * w + h), D.random_films(w, h, seed=11 * w + h + 1000)


@pytest.mark.parametrize("k", [0.2, 0.45, 1.0])
@pytest.mark.parametrize("r,f", RF, ids=[f"r{r}f{f}" for r, f in RF])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_emulated_kernels_match_the_f64_statement(emu, w, h, r, f, k):
    (even, odd), (ga, gb) = films_and_guide(w, h)
    valid, gvalid = D.resolve(even, odd)[0], D.resolve(ga, gb)[0]
    assert valid.any() and (~valid).any() and gvalid.any() and (~gvalid).any() and (valid != gvalid).any()
    out = G.run_guided(emu, even, odd, ga, gb, r, f, k)
    G.assert_guided(out, even, odd, ga, gb, r, f, k, f"{w}x{h} r={r} f={f} k={k}")
    assert len(D.range_violations(out[..., :3], even, odd, r, where=valid & gvalid)) == 0


@pytest.mark.parametrize("r,f", RF, ids=[f"r{r}f{f}" for r, f in RF])
def test_the_films_as_their_own_guide_give_the_plain_filters_bits(emu, r, f):
    plain = EF.denoise_lib()
    for w, h in SIZES:
        even, odd = D.random_films(w, h, seed=11 * w + h)
        want = EF.denoise(plain, even, odd, r, f, 0.45)
        aliased = G.run_guided(emu, even, odd, even, odd, r, f, 0.45)   # the same buffers
        copied = G.run_guided(emu, even, odd, even.copy(), odd.copy(), r, f, 0.45)
        for got in (aliased, copied):
            assert (bits(got) == bits(want)).all(), (w, h, int((bits(got) != bits(want)).sum()))
    # ... and the numpy statement with the films as the guide is _denoise_ref's, operation for operation
    assert (bits(G.guided(even, odd, even, odd, r, f, 0.45, F32)) == bits(D.denoise(even, odd, r, f, 0.45, F32))).all()


@pytest.mark.parametrize("r,f", RF, ids=[f"r{r}f{f}" for r, f in RF])
def test_two_passes_are_halves_followed_by_guided(emu, r, f):
    guide = EF.guide_lib()
    for (w, h), (r2, f2, k2) in zip(SIZES, [(1, 0, 0.45), G.DEFAULTS2, (7, 3, 0.7)]):
        even, odd = D.random_films(w, h, seed=11 * w + h)
        fa, fb = EF.guide_halves(guide, even, odd, r, f, 0.45)
        want = G.run_guided(emu, even, odd, fa, fb, r2, f2, k2)
        got = G.run_two_pass(emu, even, odd, r, f, 0.45, r2, f2, k2)
        assert (bits(got) == bits(want)).all(), (w, h, int((bits(got) != bits(want)).sum()))
    G.assert_two_pass(got, even, odd, r, f, 0.45, r2, f2, k2, f"two passes {w}x{h} r={r} f={f}, then r={r2} f={f2} k={k2}")
    assert len(D.range_violations(got[..., :3], even, odd, r2)) == 0


def test_scratch_bytes(emu):
    for fn, per_pixel in ((emu.emu_guided_scratch_bytes, 96), (emu.emu_two_pass_scratch_bytes, 128)):
        assert fn(0, 5) == 0 and fn(5, 0) == 0 and fn(67, 45) == 67 * 45 * per_pixel and fn(65535, 65535) == 65535 * 65535 * per_pixel


def test_the_range_check_has_teeth(emu):
    (even, odd), (ga, gb) = films_and_guide(41, 37)
    where = G.sure_pixels(even, odd, ga, gb)
    out = G.run_guided(emu, even, odd, ga, gb, 3, 1, 1.0)
    assert len(D.range_violations(out[..., :3], even, odd, 3, where=where)) == 0
    y, x = np.argwhere(where)[len(np.argwhere(where)) // 2]
    out[y, x, 1] += 1.5   # (the films' colours lie in [0, 1.7])
    assert D.range_violations(out[..., :3], even, odd, 3, where=where).tolist() == [[y, x]]


def test_a_constant_colour_stays(emu):
    """one colour under arbitrary positive weights in both films, whatever the guide shows: the output is the colour within the range bound"""
    rng = np.random.default_rng(4)
    h, w = 30, 50
    colour = np.array([0.8, 0.25, 0.6], F32)
    films = []
    for _ in range(2):
        wgt = rng.uniform(0.1, 50.0, (h, w, 1)).astype(F32)
        films.append(np.concatenate([colour * wgt, wgt], -1).astype(F32))
    ga, gb = D.random_films(w, h, seed=8)
    where = G.sure_pixels(films[0], films[1], ga, gb)
    for r, f in [(1, 0), (5, 1), (10, 3)]:
        out = G.run_guided(emu, films[0], films[1], ga, gb, r, f, 1.0)
        assert len(D.range_violations(out[..., :3], films[0], films[1], r, where=where)) == 0
        assert np.abs(out[where][:, :3] - colour).max() <= (2 * (2 * r + 1) ** 2 + 4) * 2.0 ** -24 * 0.8 + 2.0 ** -23   # (+ the rounding of rgb w / w)
        two = G.run_two_pass(emu, films[0], films[1], 7, 3, 0.45, r, f, 1.0)
        assert np.abs(two[..., :3] - colour).max() <= (2 * (2 * r + 1) ** 2 + 4) * 2.0 ** -24 * 0.8 + 2.0 ** -23


def test_films_or_a_guide_without_a_valid_pixel_give_zeros(emu):
    h, w = 19, 35
    (even, odd), (ga, gb) = films_and_guide(w, h)
    dead = np.zeros((h, w, 4), F32)
    dead[..., :3] = 3.0   # (colour without weight)
    nan = np.full((h, w, 4), np.nan, F32)
    for r, f in [(2, 0), (7, 3)]:
        for films in ((dead, dead.copy(), ga, gb), (even, odd, dead, dead.copy()), (even, odd, nan, nan.copy()), (even, odd, ga, -np.abs(gb))):
            out = G.run_guided(emu, *films, r, f, 1.0)
            assert (out[..., :3] == 0).all() and (out[..., 3] == 1.0).all() and np.isfinite(out).all()
        out = G.run_two_pass(emu, dead, dead.copy(), r, f, 0.45, *G.DEFAULTS2)
        assert (out[..., :3] == 0).all() and (out[..., 3] == 1.0).all()


def test_a_hole_of_the_values_is_filled_through_the_guide(emu):
    """pixels invalid in the values and valid in the guide: they take part in patches (the guide's validity), every weight they collect comes
    from the valid pixels of their window, and the output lies in that window's range"""
    rng = np.random.default_rng(6)
    h, w = 33, 47
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([0.5 + 0.3 * np.sin(xx / 9.0 + c) * np.cos(yy / 11.0) for c in range(3)], -1)
    film = lambda noise: np.concatenate([base * rng.uniform(1 - noise, 1 + noise, (h, w, 3)), np.ones((h, w, 1))], -1).astype(F32)
    even, odd, ga, gb = film(0.2), film(0.2), film(0.02), film(0.02)
    holes = [(0, 0), (16, 23), (16, 24), (32, 46), (9, 40)]
    for i, (y, x) in enumerate(holes):
        (even if i % 2 else odd)[y, x] = (0.0, np.nan, -1.0)[i % 3]
    where = np.zeros((h, w), bool)
    where[tuple(zip(*holes))] = True
    assert not (D.resolve(even, odd)[0] & where).any() and D.resolve(ga, gb)[0].all()
    for r, f in [(3, 1), (5, 1), (7, 3)]:
        out = G.run_guided(emu, even, odd, ga, gb, r, f, 1.0)
        G.assert_guided(out, even, odd, ga, gb, r, f, 1.0, f"holes r={r} f={f}")
        assert (out[where][:, :3] > 0).all()
        assert len(D.range_violations(out[..., :3], even, odd, r, where=where)) == 0
        assert np.abs(out[where][:, :3] - base[where]).max() < 0.1   # (the noise is 0.2 x 0.8 at most: a mean, not a single value)
    # the two-pass call fills them too: the first pass fills the pilot, the second finds it valid
    out = G.run_two_pass(emu, even, odd, 7, 3, 0.45, *G.DEFAULTS2)
    assert np.abs(out[where][:, :3] - base[where]).max() < 0.1 and len(D.range_violations(out[..., :3], even, odd, 5, where=where)) == 0


# ---- it is better: films of the oracle (test_denoise_emu's setup)

W = H = 64
SPP, SPLIT, REF_SPP = 32, 16, 2048
SEED, REF_SEED = 7, 1234


@pytest.mark.parametrize("name", ["cornell_box", "smallpt"])
def test_two_passes_denoise_oracle_films_better_than_one(emu, name, tmp_path, built):
    scenes.write_assets(str(tmp_path))
    p = os.path.join(str(tmp_path), "s.json")
    with open(p, "w") as fh:
        json.dump(getattr(scenes, name)(W, H, SPP), fh)
    scene, *_ = T.Scene.load_file(p)
    flat = scene.flatten(0)
    even, odd = (R.oracle_range(flat, R.tile_queue(W, H), rng, SPP, SEED)[0] for rng in ((0, SPLIT), (SPLIT, SPP)))
    ref = rgb(O.render_tiles(flat, REF_SPP, seed=REF_SEED)[0])
    r, f, k = 7, 3, 0.45
    one = EF.denoise(EF.denoise_lib(), even, odd, r, f, k)
    two = G.run_two_pass(emu, even, odd, r, f, k, *G.DEFAULTS2)
    G.assert_two_pass(two, even, odd, r, f, k, *G.DEFAULTS2, f"{name} oracle films, two passes")
    e0, e1, e2 = rmse(rgb(even + odd), ref), rmse(one[..., :3], ref), rmse(two[..., :3], ref)
    print(f"{name} {W}x{H} {SPP} spp: RMSE(noisy) = {e0:.5f}, RMSE(one pass) = {e1:.5f}, RMSE(two passes) = {e2:.5f}, ratio {e2 / e1:.3f}")
    assert e2 < e1 < e0
