"""The first-hit films and the demodulated call on the GPU (tray_render_first_hit_device, tray_debug_first_hit, tray_denoise_demodulated_device,
Hip.render_first_hit, Hip.denoise(albedo=...), Hip.render_denoised(demodulate=True)).

The per-sample records and the films are held against the statement of include/trayhip.h evaluated with the oracle (tests/_first_hit_ref.py),
the w planes also against tray_render_samples_device's film of the same samples; ranges add up, two calls agree, the host emulation's words
are compared as a finding; the demodulated call lies under the numpy statement's bar between guard bytes and gives tray_denoise_device's bits
for an albedo film without weight; a textured scene denoises better with demodulate=True; and one 1920 x 1080 call."""
import numpy as np
import pytest

import tray_rust_amd as T
from tray_rust_amd import scenes
import _denoise_ref as D
import _first_hit_ref as R
import _guided_ref as G
import _ranges
from _denoise_ref import F32, denoise_guarded, rgb, rmse

pytestmark = pytest.mark.gpu

SPP, SEED = 16, 7
W, H = 48, 32
N_ITEMS = 20000
PARTITION = [(0, 5), (5, 13), (13, 16)]
bits = lambda x: np.ascontiguousarray(x).view(np.uint32)


@pytest.fixture(scope="module")
def built_scenes(tmp_path_factory, built):
    return R.build_scenes(str(tmp_path_factory.mktemp("first_hit_gpu")), W, H, SPP)


def random_items(seed):
    rng = np.random.default_rng(seed)
    return rng.integers(0, W, N_ITEMS).astype(np.uint32), rng.integers(0, H, N_ITEMS).astype(np.uint32), rng.integers(0, SPP, N_ITEMS).astype(np.uint32)


@pytest.mark.parametrize("name", R.STATIC + R.MOVING)
def test_every_word_of_20000_samples_is_the_statements(built_scenes, name):
    scene, frame = built_scenes[name]
    items = random_items(5)
    got = R.gpu_records(scene, frame, *items, SPP, SEED)
    R.assert_records(got, R.records(scene.flatten(frame), *items, SPP, SEED), name)
    # the emulation against the GPU: a finding, not a bar
    emu = R.emu_records(scene.flatten(frame), *items, SPP, SEED)
    print(f"{name}: {int((bits(emu) != bits(got)).sum())} of {emu.size} words of the host emulation differ from the GPU's")


def reference_films(scene, frame, w, h, rng, tiles=None):
    flat = scene.flatten(frame)
    q = _ranges.tile_queue(w, h)
    q = q if tiles is None else q[tiles[0]:tiles[0] + tiles[1]]
    items = R.frame_items(q, SPP)
    m = (items[2] >= rng[0]) & (items[2] < rng[1])
    items = tuple(v[m] for v in items)
    return R.films_of(flat, q, items, R.records(flat, *items[:3], SPP, SEED), rng)


def check_films(scene, frame, w, h, rng, what, tiles=None):
    got, _ = R.gpu_films(scene, frame, SPP, rng, SEED, tiles or (0, 0))
    R.assert_films_match(got, reference_films(scene, frame, w, h, rng, tiles), what)
    for other in got[1:]:   # one weight plane of the window, flushed three times: the same sums up to the order of the workgroups' atomics
        assert np.abs(other[..., 3] - got[0][..., 3]).max() <= 2e-5 * max(1.0, float(got[0][..., 3].max()))
    colour = R.gpu_colour_film(scene, frame, SPP, rng, SEED, tiles or (0, 0))
    t = colour[..., 3] != 0
    assert ((got[0][..., 3] != 0) == t).all(), f"{what}: the colour film touches other pixels"
    wr = (np.abs(got[0][..., 3] - colour[..., 3])[t] / np.abs(colour[..., 3][t])).max()
    print(f"{what}: w against tray_render_samples_device's film: {wr:.2e} relative")
    assert wr <= 2e-5
    return got


@pytest.mark.parametrize("name", ["textured_box", "open_cornell", "moving_box"])
def test_films_at_48x32(built_scenes, name):
    scene, frame = built_scenes[name]
    for rng in [(0, 1), (5, 13)]:
        check_films(scene, frame, W, H, rng, f"{name} {W}x{H} range {rng}")
    got = check_films(scene, frame, W, H, (0, 5), f"{name} tiles (3, 5)", tiles=(3, 5))
    assert (got[0][..., 3] == 0).any()   # pixels outside the subset's footprint


def test_films_at_64x64(tmp_path, built):
    scene = T.Scene.load_file(scenes.write_textured_box(str(tmp_path), width=64, height=64, samples=SPP))[0]
    check_films(scene, 0, 64, 64, (13, 16), "textured_box 64x64 range (13, 16)")
    check_films(scene, 0, 64, 64, (0, SPP), "textured_box 64x64, the whole frame")


@pytest.mark.parametrize("name", ["textured_box", "moving_box", "tr15_like"])
def test_ranges_add_up_and_two_calls_agree(built_scenes, name):
    scene, frame = built_scenes[name]
    whole, _ = R.gpu_films(scene, frame, SPP, (0, SPP), SEED)
    again, _ = R.gpu_films(scene, frame, SPP, (0, SPP), SEED)
    R.assert_sum_matches(again, whole, f"{name}: two calls")
    one, dev = None, None
    for rng in PARTITION:   # (into one film, as both halves of a render may)
        one, dev = R.gpu_films(scene, frame, SPP, rng, SEED, into=dev)
    R.assert_sum_matches(one, whole, f"{name}: three ranges in one film")
    cfg = T.Config(".", "", SPP, 1, T.FrameInfo(2, 0.0, 0, 1))
    cfg.current_frame = frame
    via_python = T.Hip(0, seed=SEED).render_first_hit(scene, cfg)
    R.assert_sum_matches([via_python[k] for k in R.NAMES], whole, f"{name}: Hip.render_first_hit")


SIZES = [(5, 3), (67, 45)]


@pytest.mark.parametrize("passes", [1, 2])
@pytest.mark.parametrize("rf", [(1, 0), (7, 3)])
def test_demodulated_call_is_under_the_statements_bar(built, rf, passes):
    second = G.DEFAULTS2 if passes == 2 else None
    for w, h in SIZES:
        even, odd = D.random_films(w, h, 11)
        albedo = R.random_albedo(w, h, 12)
        got = R.demodulated_guarded(even, odd, albedo, *rf, 0.45, second)
        R.assert_demodulated(got, even, odd, albedo, *rf, 0.45, second, f"gpu {w}x{h} r={rf[0]} f={rf[1]} passes={passes}")
        again = R.demodulated_guarded(even, odd, albedo, *rf, 0.45, second)
        assert (bits(got) == bits(again)).all(), "two calls differ"
        via_python = T.Hip(0).denoise(even, odd, *rf, 0.45, passes=passes, albedo=albedo)
        assert (bits(via_python) == bits(got)).all()
        emu = R.emu_demodulated(even, odd, albedo, *rf, 0.45, second)
        print(f"{w}x{h}: {int((bits(emu) != bits(got)).sum())} of {emu.size} words of the host emulation differ from the GPU's")


def test_an_albedo_film_without_weight_gives_tray_denoise_devices_bits(built):
    w, h = 67, 45
    even, odd = D.random_films(w, h, 5)
    plain = denoise_guarded(even, odd, 7, 3, 0.45)
    two = G.two_pass_guarded(even, odd, 7, 3, 0.45, *G.DEFAULTS2)
    for albedo in (np.zeros((h, w, 4), F32), np.full((h, w, 4), np.nan, F32)):
        assert (bits(R.demodulated_guarded(even, odd, albedo, 7, 3, 0.45)) == bits(plain)).all()
        assert (bits(R.demodulated_guarded(even, odd, albedo, 7, 3, 0.45, G.DEFAULTS2)) == bits(two)).all()


def test_demodulate_denoises_a_rendered_textured_scene_better(tmp_path, built):
    w, h, spp = 160, 96, 32
    scene, rt, _, fi = T.Scene.load_file(scenes.write_textured_box(str(tmp_path), width=w, height=h, samples=spp))
    hip = T.Hip(0, seed=SEED)
    cfg = T.Config(str(tmp_path), "textured_box.json", spp, 1, fi)
    shown = []
    for kw in (dict(), dict(demodulate=True), dict(demodulate=True, feature_spp=4)):
        rt.clear()
        hip.render_denoised(scene, rt, cfg, **kw)
        shown.append(np.array(rt.get_renderf32()).reshape(h, w, 4)[..., :3].copy())
    scene.release_device()
    ref = D.reference_image(scene, 4096, seed=1234)
    e1, e2, e3 = (rmse(x, ref) for x in shown)
    print(f"textured_box {w}x{h} {spp} spp: RMSE(plain) = {e1:.5f}, RMSE(demodulated) = {e2:.5f}, ratio {e2 / e1:.3f}; "
          f"albedo from 4 samples: {e3:.5f}, ratio {e3 / e1:.3f}")
    assert e2 < e1


def test_full_size_call(tmp_path, built):
    """1920 x 1080, 8 samples of cornell_box: weight for weight with the colour film, the resolved albedo within the filter's overshoot of [0, 1]"""
    w, h = 1920, 1080
    scenes.write_assets(str(tmp_path))
    scene = R.load_scene(str(tmp_path), "big", scenes.cornell_box, w, h, SPP)
    (albedo, normal, depth), _ = R.gpu_films(scene, 0, SPP, (0, 8), SEED)
    colour = R.gpu_colour_film(scene, 0, SPP, (0, 8), SEED)
    t = colour[..., 3] != 0
    assert t.all() and ((albedo[..., 3] != 0) == t).all()
    assert (np.abs(albedo[..., 3] - colour[..., 3]) / np.abs(colour[..., 3])).max() <= 2e-5
    a = albedo[..., :3] / albedo[..., 3:]
    print(f"1920x1080: resolved albedo in [{a.min():.4f}, {a.max():.4f}], coverage {float((depth[..., 1] / depth[..., 3]).mean()):.4f}")
    assert a.min() >= -0.05 and a.max() <= 1.05
    assert np.isfinite(normal).all() and np.isfinite(depth).all()
