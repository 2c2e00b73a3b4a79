"""tray_denoise_device's kernels (denoise_kernels.h) in the host emulation, against the numpy statement of the filter (tests/_denoise_ref.py,
which restates include/trayhip.h in float32 and float64).

tests/emu/emu_denoise.cpp runs k_dn_prepare and k_dn_filter as SIMT fibers: the LDS staging, the two barriers per offset and the separable
patch sums execute as on the device. The bar of every comparison is _denoise_ref.bar: the kernels may differ from the f64 statement by 4 x what
the f32 numpy statement differs from it on the same input, plus 1e-7 (they sum 49 patch terms and up to 441 weights in another order than
numpy); validity decisions agree exactly. Then the properties the header states (range, a noise-free film, a constant colour, degenerate
films), and that the filter denoises films of the oracle: RMSE(denoised) / RMSE(even + odd) against a 2048-spp oracle render is 0.598 on
cornell_box and 0.568 on smallpt (64 x 64, 32 spp, the defaults); the condition is < 1."""
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
from _denoise_ref import rgb, rmse
from _emu_features import denoise as run

F32 = np.float32


@pytest.fixture(scope="module")
def emu():
    return EF.denoise_lib()


SIZES = [(5, 3), (20, 12), (67, 45)]   # smaller than a window; not multiples of the 32 x 16 tile
RF = [(1, 0), (3, 1), (7, 3), (10, 3)]


@pytest.mark.parametrize("k", [0.2, 0.45, 1.0])
@pytest.mark.parametrize("r,f", RF, ids=[f"r{r}f{f}" for r, f in RF])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_emulated_kernels_match_the_f64_statement(emu, w, h, r, f, k):
    even, odd = D.random_films(w, h, seed=11 * w + h)
    valid = D.resolve(even, odd)[0]
    assert (~valid).any() and valid.any()
    cy, cx = h - 2, w - 3   # (random_films: the valid pixel whose 3 x 3 box is otherwise invalid)
    assert valid[cy, cx] and valid[cy - 1:cy + 2, cx - 1:cx + 2].sum() == 1
    out = run(emu, even, odd, r, f, k)
    D.assert_matches(out, even, odd, r, f, k, f"{w}x{h} r={r} f={f} k={k}")
    assert len(D.range_violations(out[..., :3], even, odd, r)) == 0


def test_scratch_bytes_cover_three_records_per_pixel(emu):
    assert emu.emu_denoise_scratch_bytes(0, 5) == 0 and emu.emu_denoise_scratch_bytes(5, 0) == 0
    assert emu.emu_denoise_scratch_bytes(67, 45) == 67 * 45 * 48


# ---- properties

@pytest.mark.parametrize("r,f", [(3, 1), (7, 3)])
def test_range_property(emu, r, f):
    """every output channel of a valid pixel lies between the extremes of a and b over the valid pixels of its window (_denoise_ref.range_violations)"""
    even, odd = D.random_films(41, 37, seed=5)
    out = run(emu, even, odd, r, f, 0.45)
    bad = D.range_violations(out[..., :3], even, odd, r)
    assert len(bad) == 0, bad[:8].tolist()
    # the check itself sees a value pushed out of the window's range
    valid = D.resolve(even, odd)[0]
    y, x = np.argwhere(valid)[7]
    out[y, x, 1] = 50.0
    assert [y, x] in D.range_violations(out[..., :3], even, odd, r).tolist()


def test_a_noise_free_film_is_left_alone(emu):
    """identical halves: V = 0 and t = diff^2 / eps, so for i.i.d. uniform colours every foreign weight underflows and out.rgb == a to the bit"""
    rng = np.random.default_rng(3)
    h, w = 24, 40
    col = rng.uniform(0.05, 1.0, (h, w, 3)).astype(F32)
    wgt = rng.uniform(0.5, 4.0, (h, w, 1)).astype(F32)
    film = np.concatenate([col * wgt, wgt], -1).astype(F32)
    for r, f in [(3, 1), (7, 3)]:
        lowest = []
        D.denoise(film, film, r, f, 0.45, np.float64, min_foreign_d2=lowest)
        assert lowest[0] > 104.0, lowest   # exp(-x) is 0 in f32 for x > 103.98
        out = run(emu, film, film.copy(), r, f, 0.45)
        a = D.resolve(film, film)[1]
        assert (out[..., :3].view(np.uint32) == a.view(np.uint32)).all()
        assert (out[..., 3] == 1.0).all()


def test_a_constant_colour_stays(emu):
    """one colour under arbitrary positive weights in both films: every weight is 1, the output is the colour within the range bound"""
    rng = np.random.default_rng(4)
    h, w = 30, 50
    colour = np.array([0.8, 0.25, 0.6], F32)
    films = []
    for _ in range(2):
        wgt = rng.uniform(0.1, 50.0, (h, w, 1)).astype(F32)
        films.append(np.concatenate([colour * wgt, wgt], -1).astype(F32))
    for r, f in [(1, 0), (7, 3), (10, 3)]:
        out = run(emu, films[0], films[1], r, f, 0.45)
        assert len(D.range_violations(out[..., :3], films[0], films[1], r)) == 0
        assert np.abs(out[..., :3] - colour).max() <= (2 * (2 * r + 1) ** 2 + 4) * 2.0 ** -24 * 0.8 + 2.0 ** -23   # (+ the rounding of rgb w / w)


def test_degenerate_films(emu):
    h, w = 19, 35
    zero = np.zeros((h, w, 4), F32)
    for r, f in [(2, 0), (7, 3)]:
        out = run(emu, zero, zero.copy(), r, f, 0.45)
        assert (out[..., :3] == 0).all() and (out[..., 3] == 1.0).all()
        even, odd = zero.copy(), zero.copy()
        even[..., :3] = 3.0; odd[..., 3] = -1.0   # (colour without weight, negative weight: still all invalid)
        even[9, 17], odd[9, 17] = (0.5, 1.0, 1.5, 2.0), (0.75, 0.5, 0.25, 1.0)
        out = run(emu, even, odd, r, f, 0.45)
        a, b = even[9, 17, :3] / even[9, 17, 3], odd[9, 17, :3] / odd[9, 17, 3]
        assert (out[9, 17, :3] == (a + b) * F32(0.5)).all(), out[9, 17]
        rest = np.ones((h, w), bool); rest[9, 17] = False
        assert (out[rest][:, :3] == 0).all() and np.isfinite(out).all()


# ---- it denoises: films of the oracle

W = H = 64
SPP, SPLIT, REF_SPP = 32, 16, 2048
SEED, REF_SEED = 7, 1234


@pytest.mark.parametrize("name", ["cornell_box", "smallpt"])
def test_it_denoises_oracle_films(emu, name, tmp_path, built):
    scenes.write_assets(str(tmp_path))
    p = os.path.join(str(tmp_path), "s.json")
    with open(p, "w") as fh:
        json.dump(getattr(scenes, name)(W, H, SPP), fh)
    scene, *_ = T.Scene.load_file(p)
    flat = scene.flatten(0)
    even, odd = (R.oracle_range(flat, R.tile_queue(W, H), rng, SPP, SEED)[0] for rng in ((0, SPLIT), (SPLIT, SPP)))
    ref = rgb(O.render_tiles(flat, REF_SPP, seed=REF_SEED)[0])
    r, f, k = 7, 3, 0.45
    out = run(emu, even, odd, r, f, k)
    D.assert_matches(out, even, odd, r, f, k, f"{name} oracle films")
    noisy, clean = rmse(rgb(even + odd), ref), rmse(out[..., :3], ref)
    print(f"{name} {W}x{H} {SPP} spp: RMSE(even + odd) = {noisy:.5f}, RMSE(denoised) = {clean:.5f}, ratio {clean / noisy:.3f}")
    assert clean < noisy
    # five pixels made invalid as a noise-target border defect would: the filter fills them
    holes = [(5, 9), (20, 33), (40, 12), (41, 12), (60, 60)]
    e2, o2 = even.copy(), odd.copy()
    e2[5, 9, 3] = 0.0; o2[20, 33, 3] = -1.0; e2[40, 12, 3] = np.nan; o2[41, 12, 1] = np.nan; e2[60, 60] = 0.0
    out2 = run(emu, e2, o2, r, f, k)
    assert np.isfinite(out2).all()
    where = np.zeros((H, W), bool)
    for y, x in holes:
        where[y, x] = True
    assert not D.resolve(e2, o2)[0][where].any()
    assert len(D.range_violations(out2[..., :3], e2, o2, r, where=where)) == 0
    filled = np.array([out2[y, x, :3] for y, x in holes])
    print(f"{name}: the five filled pixels lie within {np.abs(filled - np.array([ref[y, x] for y, x in holes])).max():.4f} of the reference")
    assert rmse(out2[..., :3], ref) < noisy
