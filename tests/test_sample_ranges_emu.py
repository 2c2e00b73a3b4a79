"""Sample ranges (tray_render_samples_device) in the host emulation of the device source, against the oracle.

tests/emu/emu_sample_ranges.cpp adds range entry points to the emulation: the tile kernel (row-binned film on and off, and cut into
progressive slices), the wavefront schedule (4 chunks, and TRAYHIP_WF_SLICES=4) and the sampler pass on an AnimatedMesh, each handed
[begin, end) of a 16-sample LowDiscrepancy frame as device_api.hip hands it. A range's film must be RenderTarget::write of exactly the
samples begin .. end - 1 of every pixel -- sample s traced as the whole frame traces it -- with the counts of those samples, and the
films of ranges that partition [0, spp) must add up to the whole frame. Bars as tests/test_film_footprints.py: equal touched pixels,
per-pixel weight within 2e-5 of the pixel's own."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

import tray_rust_amd as T
from tray_rust_amd import _lib as L
from tray_rust_amd import scenes
import _emu as E
import _oracle as O

SPP = 16
RANGES = [(0, 5), (5, 13), (13, 16), (7, 8)]   # three that partition [0, 16) (none a power of two long but the middle one), and one sample
PARTITION = RANGES[:3]
W, H = 16, 16
SEED = 7


def _lib():
    so = os.path.join(E.EMU_DIR, "libtrayemu_ranges.so")
    src = os.path.join(E.EMU_DIR, "emu_sample_ranges.cpp")
    _, deps, cmd = E._target(())
    deps = deps + [src]
    if E._stale(so, deps):
        cmd = [so if a == cmd[cmd.index("-o") + 1] else a for a in cmd]
        cmd[cmd.index(os.path.join(E.EMU_DIR, "emu_kernels.cpp"))] = src
        subprocess.run(cmd, check=True)
    h = C.CDLL(so)
    FS = C.POINTER(L.TrayFlatScene)
    h.emu_render_tiles_range.restype = C.c_int
    h.emu_render_tiles_range.argtypes = [FS, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32,
                                         C.c_int, C.c_int, C.c_void_p]
    h.emu_render_wavefront_range.restype = C.c_int
    h.emu_render_wavefront_range.argtypes = [FS, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32,
                                             C.c_uint32, C.c_void_p]
    h.emu_render_sampler_range.restype = C.c_int
    h.emu_render_sampler_range.argtypes = [FS, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32,
                                           C.c_void_p]
    return h


@pytest.fixture(scope="module")
def emu_ranges(built):
    return _lib()


def tile_queue(width, height):
    return np.array(T.BlockQueue((width, height), (8, 8)).blocks, np.uint32).reshape(-1, 2)


def render_range(h, kind, flat, q, rng, **kw):
    """one range launch in the emulation; returns (rgbw image, (samples, vertices, rays))"""
    fs = flat.contents
    img = np.zeros((fs.film.height, fs.film.width, 4), np.float32)
    st = np.zeros(4, np.uint64)
    q = np.ascontiguousarray(q, np.uint32)
    if kind == "tiles":
        rc = h.emu_render_tiles_range(flat, q.ctypes.data, len(q), SPP, rng[0], rng[1], SEED, img.ctypes.data, 2, -1, kw.get("film_rows", -1), st.ctypes.data)
    elif kind == "wavefront":
        rc = h.emu_render_wavefront_range(flat, q.ctypes.data, len(q), SPP, rng[0], rng[1], SEED, img.ctypes.data, 4, 2, st.ctypes.data)
    else:
        rc = h.emu_render_sampler_range(flat, q.ctypes.data, len(q), SPP, rng[0], rng[1], SEED, img.ctypes.data, 0, st.ctypes.data)
    assert rc == 0, f"{kind} range {rng}: {rc}"
    return img, tuple(int(v) for v in st[:3])


def oracle_range(flat, q, rng):
    """the oracle's film of the samples [begin, end) of every pixel of the tiles q: oracle_sample_radiance for the samples (clamped colour,
    film position, vertices, rays), oracle_film_patches for RenderTarget::write of each; returns (rgbw image, (samples, vertices, rays))"""
    fs = flat.contents
    w, h = fs.film.width, fs.film.height
    r = E.FILM_PATCH_R
    pad = np.zeros((h + 2 * r, w + 2 * r, 4), np.float32)
    counts = np.zeros(3, np.int64)
    for tile in q:
        px, py = np.meshgrid(np.arange(8) + 8 * int(tile[0]), np.arange(8) + 8 * int(tile[1]))
        px, py = np.repeat(px.ravel(), rng[1] - rng[0]), np.repeat(py.ravel(), rng[1] - rng[0])
        si = np.tile(np.arange(rng[0], rng[1]), 64)
        out = O.sample_radiance(flat, px, py, si, SPP, seed=SEED)
        counts += (len(out), int(out[:, 5].sum()), int(out[:, 6].sum()))
        s = np.concatenate([out[:, 3:5], out[:, 0:3]], 1)
        patches = O.film_patches(fs.film, (int(tile[0]), int(tile[1])), s, r)
        for (x, y), p in zip(np.floor(out[:, 3:5]).astype(int), patches):
            pad[y:y + 2 * r + 1, x:x + 2 * r + 1] += p   # (patch pixel (r, r) is the sample's own pixel; pad shifts by r)
    return pad[r:r + h, r:r + w], tuple(int(c) for c in counts)


def assert_film_matches(img, ref, what):
    """touched pixels equal; weight per pixel within 2e-5 of the pixel's own weight (tests/test_film_footprints.py)"""
    t_img, t_ref = img[..., 3] != 0, ref[..., 3] != 0
    assert (t_img == t_ref).all(), f"{what}: touched pixels differ at {np.argwhere(t_img != t_ref)[:8].tolist()}"
    wr = np.abs(img[..., 3] - ref[..., 3])[t_ref] / np.abs(ref[..., 3][t_ref])
    assert wr.max() <= 2e-5, f"{what}: per-pixel relative weight difference {wr.max():.2e} on {int((wr > 2e-5).sum())} px"
    full = ref[..., 3] >= 0.1 * ref[..., 3].max()
    a = img[..., :3][full] / img[..., 3:][full]
    b = ref[..., :3][full] / ref[..., 3:][full]
    assert np.abs(a - b).max() < 2e-5, what


@pytest.fixture(scope="module")
def cornell(tmp_path_factory, built):
    d = str(tmp_path_factory.mktemp("ranges"))
    scenes.write_assets(d)
    p = os.path.join(d, "cornell.json")
    with open(p, "w") as f:
        json.dump(scenes.cornell_box(W, H, SPP), f)
    scene, *_ = T.Scene.load_file(p)
    flat = scene.flatten(0)
    refs = {rng: oracle_range(flat, tile_queue(W, H), rng) for rng in RANGES}
    return scene, flat, refs


@pytest.fixture(scope="module")
def flag(tmp_path_factory, built):
    d = str(tmp_path_factory.mktemp("flag"))
    path = scenes.write_waving_flag(d, grid=6, n_keys=3, width=W, height=H, samples=SPP, frames=4, scene_time=2.0)
    scene, *_ = T.Scene.load_file(path)
    flat = scene.flatten(1)
    refs = {rng: oracle_range(flat, tile_queue(W, H), rng) for rng in RANGES}
    return scene, flat, refs


def test_oracle_range_films_add_up_to_the_oracle_frame(cornell):
    """the reference films of this file: their sum over a partition is oracle_render_tiles' frame"""
    _, flat, refs = cornell
    ref, st = O.render_tiles(flat, SPP, seed=SEED)
    assert_film_matches(sum(refs[r][0] for r in PARTITION), ref, "oracle ranges")
    assert tuple(sum(np.array(refs[r][1]) for r in PARTITION)) == (st.samples, st.vertices, st.rays)


CASES = [("tiles", {"film_rows": -1}, {}), ("tiles", {"film_rows": 0}, {}), ("tiles", {"film_rows": -1}, {"TRAYHIP_TILE_SLICES": "3"}),
         ("wavefront", {}, {}), ("wavefront", {}, {"TRAYHIP_WF_SLICES": "4"})]
CASE_IDS = ["tiles-rows", "tiles-window", "tiles-3-slices", "wavefront", "wavefront-4-slices"]


@pytest.mark.parametrize("case", CASES, ids=CASE_IDS)
def test_ranges_on_cornell_box(case, cornell, emu_ranges, monkeypatch):
    kind, kw, env = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _, flat, refs = cornell
    q = tile_queue(W, H)
    total = None
    for rng in RANGES:
        img, counts = render_range(emu_ranges, kind, flat, q, rng, **kw)
        ref, ref_counts = refs[rng]
        assert counts == ref_counts, (rng, counts, ref_counts)
        assert counts[0] == len(q) * 64 * (rng[1] - rng[0])
        assert_film_matches(img, ref, f"{kind} {kw} {env} range {rng}")
        if rng in PARTITION:
            total = img if total is None else total + img
    frame, st = O.render_tiles(flat, SPP, seed=SEED)
    assert_film_matches(total, frame, f"{kind} {kw} {env}: sum of the ranges")


def test_whole_frame_as_a_range_is_the_whole_frame(cornell, emu_ranges):
    """[0, spp) is the whole-frame launch: the same film bit for bit as the emulation's plain entry point"""
    _, flat, _ = cornell
    q = tile_queue(W, H)
    img, counts = render_range(emu_ranges, "tiles", flat, q, (0, SPP))
    plain, st = E.render_tiles(flat, q, SPP, SEED, blocks=2)
    assert counts == st[:3]
    assert np.array_equal(img, plain)


def test_ranges_through_the_sampler_pass_on_an_animated_mesh(flag, emu_ranges):
    """LowDiscrepancy on a scene with an AnimatedMesh runs k_sampler_pass: SamplerPass.first / count carry the range"""
    _, flat, refs = flag
    q = tile_queue(W, H)
    total = None
    for rng in RANGES:
        img, counts = render_range(emu_ranges, "sampler", flat, q, rng)
        ref, ref_counts = refs[rng]
        assert counts == ref_counts, (rng, counts, ref_counts)
        assert_film_matches(img, ref, f"sampler pass range {rng}")
        if rng in PARTITION:
            total = img if total is None else total + img
    frame, st = O.render_tiles(flat, SPP, seed=SEED)
    assert_film_matches(total, frame, "sampler pass: sum of the ranges")
