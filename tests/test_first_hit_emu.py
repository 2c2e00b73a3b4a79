"""The first-hit kernels (tray_render_first_hit_device, tray_debug_first_hit, tray_denoise_demodulated_device) in the host emulation of the device
source (tests/emu/emu_first_hit.cpp), against the per-sample statement of include/trayhip.h evaluated with the oracle (tests/_first_hit_ref.py):
every word of every camera sample's record, the three films of sample ranges and tile subsets between guard words, ranges adding up, the
demodulated call under the numpy statement's bar with its weight-0 identity, and the point of it -- a textured scene denoises better."""
import numpy as np
import pytest

import tray_rust_amd as T
from tray_rust_amd import scenes
import _denoise_ref as D
import _emu_features as EF
import _first_hit_ref as R
import _guided_ref as G
import _oracle as O
import _ranges
from _denoise_ref import F32, rgb, rmse

SPP, SEED = 16, 7
W, H = 48, 32
RANGES = [(0, 1), (0, 5), (5, 13), (13, 16)]   # one sample (three waves idle), then three that partition [0, 16)
PARTITION = RANGES[1:]


@pytest.fixture(scope="module")
def flats(tmp_path_factory, built):
    """name -> (scene, flat scene of the frame under test): every film 48 x 32, 16 samples"""
    return {k: (s, s.flatten(fr)) for k, (s, fr) in R.build_scenes(str(tmp_path_factory.mktemp("first_hit")), W, H, SPP).items()}


_frames = {}


def frame_reference(flats, name):
    """(tiles, items, records) of the whole 16-sample frame of a scene, computed once"""
    if name not in _frames:
        flat = flats[name][1]
        q = _ranges.tile_queue(W, H)
        items = R.frame_items(q, SPP)
        _frames[name] = (q, items, R.records(flat, *items[:3], SPP, SEED))
    return _frames[name]


# ---- per-sample records

@pytest.mark.parametrize("name", R.STATIC + R.MOVING)
def test_every_word_of_every_sample_is_the_statements(flats, name):
    """the static scenes bit for bit; ANIM = 2 (spline stacks at every use) and ANIM = 3 (an AnimatedMesh) under the host's parity mode"""
    flat = flats[name][1]
    _, items, ref = frame_reference(flats, name)
    R.assert_records(R.emu_records(flat, *items[:3], SPP, SEED), ref, name)


# ---- films

def check_films(flats, name, w, h, rng, subset=None):
    scene, flat = flats[name]
    assert (flat.contents.film.width, flat.contents.film.height) == (w, h)
    q, items, rec = frame_reference(flats, name)
    tiles = q if subset is None else q[subset[0]:subset[0] + subset[1]]
    sel = np.arange(len(q)) if subset is None else np.arange(subset[0], subset[0] + subset[1])
    m = np.isin(items[3], sel)
    sub_items = tuple(v[m] for v in items[:3]) + (np.searchsorted(sel, items[3][m]).astype(np.uint32),)
    ref = R.films_of(flat, tiles, sub_items, rec[m], rng)
    got = R.emu_films(flat, tiles, SPP, rng, SEED)
    R.assert_films_match(got, ref, f"{name} {w}x{h} range {rng} tiles {subset}")
    # the three w planes are one plane
    assert np.array_equal(got[0][..., 3], got[1][..., 3]) and np.array_equal(got[0][..., 3], got[2][..., 3])
    return got


@pytest.mark.parametrize("rng", RANGES)
@pytest.mark.parametrize("name", ["cornell_box", "textured_box", "open_cornell"])
def test_films_of_sample_ranges(flats, name, rng):
    check_films(flats, name, W, H, rng)


def test_films_of_a_tile_subset(flats):
    """tiles 3 .. 7 of the queue: pixels outside their footprint stay zero (touched pixels equal the reference's)"""
    got = check_films(flats, "textured_box", W, H, (5, 13), subset=(3, 5))
    assert (got[0][..., 3] == 0).any()


@pytest.mark.parametrize("size", [(8, 8), (24, 16)])
def test_small_films(size, tmp_path, built):
    """8 x 8: one tile, the filter's halo clipped on every side; 24 x 16: six tiles"""
    w, h = size
    scenes.write_assets(str(tmp_path))
    scene = R.load_scene(str(tmp_path), "small", R.open_cornell, w, h, SPP)
    flat = scene.flatten(0)
    q = _ranges.tile_queue(w, h)
    items = R.frame_items(q, SPP)
    rec = R.records(flat, *items[:3], SPP, SEED)
    for rng in RANGES:
        R.assert_films_match(R.emu_films(flat, q, SPP, rng, SEED), R.films_of(flat, q, items, rec, rng), f"{w}x{h} range {rng}")


@pytest.mark.parametrize("name", ["cornell_box", "textured_box", "moving_box"])
def test_ranges_add_up_and_may_share_a_film(flats, name):
    flat = flats[name][1]
    q = _ranges.tile_queue(W, H)
    whole = R.emu_films(flat, q, SPP, (0, SPP), SEED)
    parts = [R.emu_films(flat, q, SPP, rng, SEED) for rng in PARTITION]
    R.assert_sum_matches([sum(p[i] for p in parts) for i in range(3)], whole, f"{name}: separate films")
    one = None
    for rng in PARTITION:
        one = R.emu_films(flat, q, SPP, rng, SEED, into=one)
    R.assert_sum_matches(one, whole, f"{name}: one film")
    # weight for weight with the colour film of the same samples
    colour = EF.render_range(EF.ranges_lib(), "tiles", flat, q, (0, 5), spp=SPP, seed=SEED)[0] if name != "moving_box" else None
    if colour is not None:
        first = R.emu_films(flat, q, SPP, (0, 5), SEED)[0]
        t = colour[..., 3] != 0
        assert ((first[..., 3] != 0) == t).all()
        assert (np.abs(first[..., 3] - colour[..., 3])[t] / np.abs(colour[..., 3][t])).max() <= 2e-5


# ---- the demodulated call

SECOND = G.DEFAULTS2


@pytest.mark.parametrize("passes", [1, 2])
@pytest.mark.parametrize("rf", [(1, 0), (7, 3)])
@pytest.mark.parametrize("size", [(5, 3), (20, 12), (67, 45)])
def test_demodulated_call_is_under_the_statements_bar(size, rf, passes, built):
    w, h = size
    even, odd = D.random_films(w, h, 11)
    albedo = R.random_albedo(w, h, 12)
    valid = (albedo[..., 3] > 0) & np.isfinite(albedo).all(-1)
    assert (~valid).any() and (albedo[valid][:, :3] == 0).any() and (albedo[valid][:, :3] < 0).any()
    second = SECOND if passes == 2 else None
    got = R.emu_demodulated(even, odd, albedo, *rf, 0.45, second)
    R.assert_demodulated(got, even, odd, albedo, *rf, 0.45, second, f"{w}x{h} r={rf[0]} f={rf[1]} passes={passes}")


@pytest.mark.parametrize("passes", [1, 2])
def test_an_albedo_film_without_weight_gives_the_plain_calls_bits(passes, built):
    w, h = 20, 12
    even, odd = D.random_films(w, h, 5)
    second = SECOND if passes == 2 else None
    plain = EF.denoise(EF.denoise_lib(), even, odd, 7, 3, 0.45) if passes == 1 else G.run_two_pass(G.guided_lib(), even, odd, 7, 3, 0.45, *SECOND)
    for albedo in (np.zeros((h, w, 4), F32), np.full((h, w, 4), np.nan, F32), -np.abs(R.random_albedo(w, h, 3))):
        got = R.emu_demodulated(even, odd, albedo, 7, 3, 0.45, second)
        assert np.array_equal(got.view(np.uint32), plain.view(np.uint32))


# ---- it is better where there is texture: films of the oracle

QW = QH = 64
QSPP, QSPLIT, REF_SPP, REF_SEED = 32, 16, 2048, 1234


def quality(name, d):
    if name == "textured_box":
        scene = T.Scene.load_file(scenes.write_textured_box(d, width=QW, height=QH, samples=QSPP))[0]
    else:
        scenes.write_assets(d)
        scene = R.load_scene(d, "q", getattr(scenes, name), QW, QH, QSPP)
    flat = scene.flatten(0)
    q = _ranges.tile_queue(QW, QH)
    even, odd = (_ranges.oracle_range(flat, q, rng, QSPP, SEED)[0] for rng in ((0, QSPLIT), (QSPLIT, QSPP)))
    items = R.frame_items(q, QSPP)
    albedo = R.films_of(flat, q, items, R.records(flat, *items[:3], QSPP, SEED), (0, QSPP), which=(0,))[0]
    assert np.array_equal(albedo[..., 3] != 0, (even + odd)[..., 3] != 0)
    ref = rgb(O.render_tiles(flat, REF_SPP, seed=REF_SEED)[0])
    r, f, k = 7, 3, 0.45
    plain = EF.denoise(EF.denoise_lib(), even, odd, r, f, k)
    demod = R.emu_demodulated(even, odd, albedo, r, f, k)
    e0, e1, e2 = rmse(rgb(even + odd), ref), rmse(plain[..., :3], ref), rmse(demod[..., :3], ref)
    print(f"{name} {QW}x{QH} {QSPP} spp: RMSE(noisy) = {e0:.5f}, RMSE(plain) = {e1:.5f}, RMSE(demodulated) = {e2:.5f}, ratio {e2 / e1:.3f}")
    return e0, e1, e2


def test_demodulation_denoises_a_textured_scene_better(tmp_path, built):
    e0, e1, e2 = quality("textured_box", str(tmp_path))
    assert e2 < e1 < e0


@pytest.mark.parametrize("name", ["cornell_box", "smallpt"])
def test_untextured_scenes_neither_gain_nor_lose(name, tmp_path, built):
    """printed only: 0.985 and 1.022 x the plain filter when this was measured"""
    quality(name, str(tmp_path))
