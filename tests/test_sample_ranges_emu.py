"""Sample ranges (tray_render_samples_device) in the host emulation of the device source, against the oracle.

tests/emu/emu_sample_ranges.cpp adds range entry points to the emulation: the tile kernel (row-binned film on and off, and cut into
progressive slices), the wavefront schedule (4 chunks, and TRAYHIP_WF_SLICES=4) and the sampler pass on an AnimatedMesh, each handed
[begin, end) of a 16-sample LowDiscrepancy frame as device_api.hip hands it. A range's film must be RenderTarget::write of exactly the
samples begin .. end - 1 of every pixel -- sample s traced as the whole frame traces it -- with the counts of those samples, and the
films of ranges that partition [0, spp) must add up to the whole frame. Bars as tests/test_film_footprints.py: equal touched pixels,
per-pixel weight within 2e-5 of the pixel's own."""
import json
import os

import numpy as np
import pytest

import tray_rust_amd as T
from tray_rust_amd import scenes
import _emu as E
import _emu_features as EF
from _emu_features import render_range
import _oracle as O
from _ranges import SEED, SPP, assert_film_matches, oracle_range, tile_queue

RANGES = [(0, 5), (5, 13), (13, 16), (7, 8)]   # three that partition [0, 16) (none a power of two long but the middle one), and one sample
PARTITION = RANGES[:3]
W, H = 16, 16


@pytest.fixture(scope="module")
def emu_ranges(built):
    return EF.ranges_lib()


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
