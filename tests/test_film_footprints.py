"""Film reconstruction at every filter footprint the device accepts (floor(2 w) <= 4), against the oracle's RenderTarget::write
(render_target.rs:77-146). The path tracer's samples already match the oracle bit for bit; these tests isolate the film.

RenderTarget::write admits a sample to the pixels of a 2 x 2 lock block [xw0, xw1) x [yw0, yw1) (clipped to the tile's write range)
only if xw0 - fpw <= s.x < xw1 + fpw and the same in y; the filter's own |d| * inv_w <= w test applies after that. For footprints
with w^2 > fpw + 1/2 (1.9, 2.25, ...) the block test decides whether a pixel one column or row further out is written.

* test_every_device_film_writes_the_reference_footprint: single samples through each device splat function (host emulation of the
  device source) against oracle_film_patches: the same pixels, and values within a few ulps (one sample has no summation order).
* test_whole_kernels_*: the tile kernel, the wavefront schedule and the sampler pass over a few footprints against the oracle's
  renders: equal counts, equal touched pixels, the weight plane per pixel within 2e-5 of the pixel's own weight (the order of the
  f32 sums gives at most a few 1e-6; a footprint error one column or row wide gives 5e-4 and more)."""
import json
import os

import numpy as np
import pytest

import tray_rust_amd as T
from tray_rust_amd import scenes
import _emu as E
import _oracle as O

WIDTHS = [0.5, 0.75, 1.0, 1.25, 1.5, 1.75, 1.87, 1.9, 2.0, 2.12, 2.2, 2.25, 2.4, 2.49]
# every width on both axes, every width against another one (w != h), and the row-binned film's h = 2 under widths that bind
PAIRS = sorted(set([(w, w) for w in WIDTHS] + [(w, WIDTHS[(i + 5) % len(WIDTHS)]) for i, w in enumerate(WIDTHS)]
                   + [(1.9, 2.0), (2.25, 2.0), (2.49, 2.0), (0.75, 2.0)]))
KINDS = ("mitchell_netravali", "gaussian")
W_IMG, H_IMG = 40, 24          # 5 x 3 tiles: no multiple of the sampler pass's 2 x 2 and 4 x 4 groups
TILES = [(0, 0), (4, 2), (1, 1), (3, 0), (4, 1), (0, 2), (2, 1)]   # corners, image edges, interior
MODES = {0: "film_splat (LDS window)", 1: "film_splat_global", 2: "film_splat_rows + resolve", 3: "film_splat_rows_global + resolve"}
GROUPS = [(1, 1), (2, 2), (4, 4)]   # film_splat_window under windows of 1, 4 and 16 tiles


def filter_json(kind, w, h):
    if kind == "gaussian":
        return {"type": "gaussian", "width": w, "height": h, "alpha": 2.0}
    return {"type": "mitchell_netravali", "width": w, "height": h, "b": 1.0 / 3.0, "c": 1.0 / 3.0}


def load_with_filter(d, filt, scene=None, name="f.json"):
    sd = scene if scene is not None else scenes.cornell_box(W_IMG, H_IMG, 1)
    sd["film"]["filter"] = filt
    p = os.path.join(d, name)
    with open(p, "w") as f:
        json.dump(sd, f)
    return T.Scene.load_file(p)


@pytest.fixture(scope="module")
def asset_dir(tmp_path_factory, built):
    d = str(tmp_path_factory.mktemp("film"))
    scenes.write_assets(d)
    return d


def tile_samples(tile, rng):
    """every pixel of the tile at fractions 0, 1/4, 1/2, 3/4 on both axes (the integral ones lie on every block bound
    xw0 - fpw and xw1 + fpw), plus random positions"""
    x0, y0 = tile[0] * 8, tile[1] * 8
    f = np.arange(32, dtype=np.float32) * np.float32(0.25)
    xs, ys = np.meshgrid(x0 + f, y0 + f)
    pos = np.stack([xs.ravel(), ys.ravel()], 1)
    pos = np.concatenate([pos, rng.uniform([x0, y0], [x0 + 8, y0 + 8], (96, 2)).astype(np.float32)])
    pos = np.minimum(pos, np.nextafter(np.float32([x0 + 8, y0 + 8]), np.float32(0)))   # samples of a pixel lie in [p, p + 1)
    rgb = rng.uniform(0.05, 4.0, (len(pos), 3)).astype(np.float32)
    return np.concatenate([pos, rgb], 1).astype(np.float32)


def compare_patches(got, want, what, ulps=4):
    """same touched pixels, values within a few ulps; returns nothing, raises with the first differing sample"""
    t_got, t_want = (got != 0).any(-1), (want != 0).any(-1)
    bad = (t_got != t_want).any((1, 2))
    if bad.any():
        i = int(np.argmax(bad))
        extra = np.argwhere(t_got[i] & ~t_want[i]) - E.FILM_PATCH_R
        missing = np.argwhere(t_want[i] & ~t_got[i]) - E.FILM_PATCH_R
        raise AssertionError(f"{what}: {int(bad.sum())} of {len(bad)} samples touch other pixels than RenderTarget::write; first: "
                             f"sample {i}, pixels (dy, dx) from its own written too: {extra.tolist()}, missed: {missing.tolist()}")
    tol = ulps * np.spacing(np.abs(want)) + 1e-30
    diff = np.abs(got - want)
    assert (diff <= tol).all(), f"{what}: values differ by up to {float((diff / tol).max()) * ulps:.1f} ulps"


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("wh", PAIRS, ids=lambda p: f"{p[0]}x{p[1]}")
def test_every_device_film_writes_the_reference_footprint(kind, wh, asset_dir):
    scene, *_ = load_with_filter(asset_dir, filter_json(kind, *wh))
    flat = scene.flatten(0)
    film = flat.contents.film
    assert film.filter_pixel_w <= 4 and film.filter_pixel_h <= 4
    rng = np.random.default_rng(11)
    rows_seen = False
    for tile in TILES:
        s = tile_samples(tile, rng)
        want = O.film_patches(film, tile, s, E.FILM_PATCH_R)
        for mode, name in MODES.items():
            got = E.film_splat(film, mode, tile, s)
            if got is None:
                assert mode in (2, 3) and wh[1] != 2.0
                continue
            rows_seen = rows_seen or mode == 2
            compare_patches(got, want, f"{name}, tile {tile}")
        for group in GROUPS:
            got = E.film_splat(film, 4, tile, s, group=group)
            compare_patches(got, want, f"film_splat_window under a {group[0]}x{group[1]} group, tile {tile}")
    assert rows_seen == (wh[1] == 2.0 and film.separable != 0)


# ---- whole kernels (host emulation) against the oracle's renders ----

KERNEL_CASES = [("mitchell_netravali", 1.5, 1.5), ("mitchell_netravali", 2.0, 2.0), ("mitchell_netravali", 1.9, 1.9),
                ("mitchell_netravali", 2.25, 2.25), ("mitchell_netravali", 1.9, 2.0), ("gaussian", 2.25, 2.0),
                ("gaussian", 2.49, 2.49), ("gaussian", 1.0, 2.0)]
KCASE_IDS = [f"{k[:5]}-{w}x{h}" for k, w, h in KERNEL_CASES]
W_K, H_K, SPP_K = 32, 24, 8


def rgb(img):
    return img[..., :3] / np.maximum(img[..., 3:], 1e-20)


def tile_queue(width, height):
    return np.array(T.BlockQueue((width, height), (8, 8)).blocks, np.uint32).reshape(-1, 2)


def assert_film_matches(img, ref, what):
    """touched pixels equal; weight per pixel within 2e-5 of the pixel's own weight; RGB as test_tile_megakernel_emulated_as_simt
    where the pixel's weight is at least a tenth of the image's (a partial render's edge pixels hold a few tails of the filter)"""
    t_img, t_ref = img[..., 3] != 0, ref[..., 3] != 0
    assert (t_img == t_ref).all(), f"{what}: touched pixels differ at {np.argwhere(t_img != t_ref)[:8].tolist()}"
    wr = np.abs(img[..., 3] - ref[..., 3])[t_ref] / np.abs(ref[..., 3][t_ref])
    print(f"{what}: per-pixel relative weight difference {wr.max():.2e} ({int((wr > 1e-4).sum())} px > 1e-4)")
    assert wr.max() <= 2e-5, f"{what}: per-pixel relative weight difference {wr.max():.2e} on {int((wr > 2e-5).sum())} px"
    full = ref[..., 3] >= 0.1 * ref[..., 3].max()
    a, b = rgb(img)[full], rgb(ref)[full]
    assert np.abs(a - b).max() < 2e-5, what
    assert float(np.sqrt(np.mean((a - b) ** 2))) < 2e-6, what


@pytest.fixture(scope="module")
def kernel_scenes(asset_dir):
    out = {}
    for (kind, w, h), cid in zip(KERNEL_CASES, KCASE_IDS):
        out[cid] = load_with_filter(asset_dir, filter_json(kind, w, h), scenes.cornell_box(W_K, H_K, SPP_K), name=cid + ".json")[0]
    return out


@pytest.mark.parametrize("cid", KCASE_IDS)
def test_whole_kernels_tile_and_wavefront(cid, kernel_scenes):
    """k_path_tiles with the row-binned film left on (taken when h = 2) and forced off, the wavefront schedule, and a shard of the tile
    queue (range edges of the chunked work-item mapping)"""
    scene = kernel_scenes[cid]
    flat = scene.flatten(0)
    q = tile_queue(W_K, H_K)
    ref, st = O.render_tiles(flat, SPP_K, seed=7)
    for film_rows in (-1, 0):
        img, (samples, vertices, rays, _) = E.render_tiles(flat, q, SPP_K, 7, blocks=2, film_rows=film_rows)
        assert (samples, vertices, rays) == (st.samples, st.vertices, st.rays)
        assert_film_matches(img, ref, f"{cid} k_path_tiles film_rows={film_rows}")
    img, (samples, vertices, rays, _) = E.render_wavefront(flat, q, SPP_K, 7, n_chunks=4)
    assert (samples, vertices, rays) == (st.samples, st.vertices, st.rays)
    assert_film_matches(img, ref, f"{cid} wavefront")
    # shard 1 of 3 with 2-tile chunks: tiles 2, 3, 8, 9 of the queue
    img, (samples, vertices, rays, _) = E.render_tiles(flat, q, SPP_K, 7, blocks=1, shard=(1, 3, 2))
    sref, counts = np.zeros_like(ref), np.zeros(3, np.int64)
    for t in (2, 3, 8, 9):
        r, sst = O.render_tiles(flat, SPP_K, seed=7, tile_start=t, tile_count=1)
        sref += r
        counts += (sst.samples, sst.vertices, sst.rays)
    assert (samples, vertices, rays) == tuple(counts)
    assert_film_matches(img, sref, f"{cid} k_path_tiles shard 1/3")


SAMPLER_CASES = ["mitch-1.9x1.9", "mitch-2.25x2.25", "gauss-2.25x2.0", "mitch-2.0x2.0"]


@pytest.mark.parametrize("cid", SAMPLER_CASES)
def test_whole_kernels_sampler_pass(cid, kernel_scenes, monkeypatch):
    """k_sampler_pass (film_splat_window) under Uniform and Adaptive(2, 8), whole groups and ragged one-tile groups"""
    flat = kernel_scenes[cid].flatten(0)
    q = tile_queue(W_K, H_K)
    for kind, args in ((O.SAMPLER_UNIFORM, (1, 1)), (O.SAMPLER_ADAPTIVE, (2, 8))):
        ref, st, _ = O.render_tiles_sampler(flat, kind, *args, seed=5)
        img, (samples, vertices, rays) = E.render_sampler(flat, q, kind, *args, seed=5)
        assert (samples, vertices, rays) == (st.samples, st.vertices, st.rays)
        assert_film_matches(img, ref, f"{cid} sampler {kind}")
    monkeypatch.setenv("TRAYHIP_SAMPLER_GROUP", "3")   # groups of three tiles: not squares, walked tile by tile
    ref, st, _ = O.render_tiles_sampler(flat, O.SAMPLER_ADAPTIVE, 2, 8, seed=5)
    img, (samples, _, _) = E.render_sampler(flat, q, O.SAMPLER_ADAPTIVE, 2, 8, seed=5)
    assert samples == st.samples
    assert_film_matches(img, ref, f"{cid} sampler adaptive, groups of 3")


@pytest.mark.parametrize("filt", [("mitchell_netravali", 1.9, 1.9), ("gaussian", 2.25, 2.0)], ids=["mitch-1.9x1.9", "gauss-2.25x2.0"])
def test_whole_kernels_sampler_pass_low_discrepancy_on_an_animated_mesh(filt, tmp_path, built):
    """scenes with an AnimatedMesh take k_sampler_pass under LowDiscrepancy as well: the tile kernel's samples through film_splat_window"""
    d = str(tmp_path)
    path = scenes.write_waving_flag(d, grid=6, n_keys=3, width=W_K, height=H_K, samples=4, frames=4, scene_time=2.0)
    with open(path) as f:
        sd = json.load(f)
    sd["film"]["filter"] = filter_json(*filt)
    with open(path, "w") as f:
        json.dump(sd, f)
    scene, *_ = T.Scene.load_file(path)
    flat = scene.flatten(1)
    ref, st = O.render_tiles(flat, 4, seed=2)
    img, (samples, vertices, rays) = E.render_sampler(flat, tile_queue(W_K, H_K), O.SAMPLER_LOW_DISCREPANCY, 4, 4, seed=2)
    assert (samples, vertices, rays) == (st.samples, st.vertices, st.rays)
    assert_film_matches(img, ref, f"{filt} animated mesh, LowDiscrepancy")
