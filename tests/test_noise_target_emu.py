"""tray_render_noise_target_device's per-round kernels (noise_kernels.h) in the host emulation, against a numpy statement of include/trayhip.h,
and range launches over scattered tile lists against the oracle.

tests/emu/emu_noise.cpp runs k_noise_error and k_noise_compact as SIMT fibers: the shuffles of the error reduction and the ballots and
barriers of the block-wide scan execute as on the device. Bars: errors within 4 ulps of the numpy metric (NaN where it is NaN), flags and
samples exact, the compacted list exactly the flagged queue entries in queue order. The rounds after the first render a list of the tiles
that are still active; the range launches of every schedule must render exactly those tiles' samples, with the bars of
tests/test_sample_ranges_emu.py."""
import json
import os

import numpy as np
import pytest

import tray_rust_amd as T
from tray_rust_amd import scenes
import _emu_features as EF
import _ranges as R   # (the oracle's film of a range and its bars)
from _emu_features import noise_error as run_error
from _noise_ref import assert_ulps, numpy_tile_error, tiles_over

F32 = np.float32


@pytest.fixture(scope="module")
def noise():
    return EF.noise_lib()


@pytest.fixture(scope="module")
def emu_ranges(built):
    return EF.ranges_lib()


def random_films(w, h, seed):
    """even / odd RGBW films whose weights and colours vary, with pixels of zero, negative and NaN weight or colour, pixels whose two halves
    agree exactly, and negative colours (m = max(0, ...) clamps)"""
    rng = np.random.default_rng(seed)
    films = []
    base = rng.gamma(2.0, 0.5, (h, w, 3)).astype(F32)
    for _ in range(2):
        wgt = rng.uniform(0.5, 8.0, (h, w)).astype(F32)
        col = (base * rng.uniform(0.7, 1.3, (h, w, 3))).astype(F32)
        films.append(np.concatenate([col * wgt[..., None], wgt[..., None]], -1).astype(F32))
    even, odd = films
    n = w * h
    pick = lambda k: np.unravel_index(rng.choice(n, k, replace=False), (h, w))
    even[pick(3)] = 0.0                        # no sample landed
    odd[pick(2)] *= -1.0                       # negative weight (filters with negative lobes)
    ys, xs = pick(2); even[ys, xs, 1] = np.nan  # a NaN colour
    ys, xs = pick(1); odd[ys, xs, 3] = np.nan   # a NaN weight
    ys, xs = pick(4); odd[ys, xs] = even[ys, xs]   # both halves agree: d = 0
    ys, xs = pick(3); even[ys, xs, :3] *= -1.0; odd[ys, xs, :3] *= -1.0   # negative colours: m clamps to 0
    return np.ascontiguousarray(even), np.ascontiguousarray(odd)


@pytest.mark.parametrize("w,h", [(20, 12), (40, 24), (64, 64)], ids=["20x12-edge-tiles", "40x24", "64x64"])
@pytest.mark.parametrize("seed", [1, 2])
def test_error_kernel_matches_the_numpy_metric(noise, w, h, seed):
    even, odd = random_films(w, h, seed)
    queue = tiles_over(w, h)
    want = np.array([numpy_tile_error(even, odd, t) for t in queue], F32)
    assert np.isinf(want).any() and np.isnan(want).any() and np.isfinite(want).any()
    # round 0: the whole queue, queue index = list index
    thr = F32(np.nanmedian(want[np.isfinite(want)]))
    err, active, samples = run_error(noise, even, odd, queue, None, 16, 64, thr, len(queue))
    assert_ulps(err, want, 4, f"{w}x{h} round 0")
    assert (samples == 16).all()
    with np.errstate(invalid="ignore"):
        assert (active == (~(want < thr)).astype(np.uint32)).all()
    # a later round: a scattered list of the queue (every third tile, from the second on); the others keep what they had
    sel = np.arange(1, len(queue), 3)
    err, active, samples = run_error(noise, even, odd, queue[sel], sel, 32, 64, thr, len(queue))
    assert_ulps(err[sel], want[sel], 4, f"{w}x{h} scattered list")
    rest = np.setdiff1d(np.arange(len(queue)), sel)
    assert (err[rest] == -1.0).all() and (active[rest] == 7).all() and (samples[rest] == 7).all()
    assert (samples[sel] == 32).all()
    with np.errstate(invalid="ignore"):
        assert (active[sel] == (~(want[sel] < thr)).astype(np.uint32)).all()


def test_threshold_is_strict_and_max_spp_ends_every_tile(noise):
    """a tile whose error equals the threshold stays active (error < threshold stops it); at n_taken == max_spp no tile does"""
    w, h = 40, 24
    even, odd = random_films(w, h, 5)
    queue = tiles_over(w, h)
    err, _, _ = run_error(noise, even, odd, queue, None, 8, 64, F32(1.0), len(queue))
    k = int(np.flatnonzero(np.isfinite(err))[0])
    _, active, _ = run_error(noise, even, odd, queue, None, 8, 64, err[k], len(queue))
    assert active[k] == 1
    _, active, _ = run_error(noise, even, odd, queue, None, 8, 64, np.nextafter(err[k], F32(np.inf)), len(queue))
    assert active[k] == 0
    _, active, _ = run_error(noise, even, odd, queue, None, 64, 64, F32(0.0), len(queue))   # threshold 0: only max_spp stops a tile
    assert (active == 0).all()
    _, active, _ = run_error(noise, even, odd, queue, None, 32, 64, F32(0.0), len(queue))
    assert (active == (~(err < 0)).astype(np.uint32)).all() and active.sum() == len(queue)


@pytest.mark.parametrize("n", [0, 1, 63, 64, 1000, 1024, 1025, 4099, 32400])
def test_compaction_keeps_queue_order(noise, n):
    rng = np.random.default_rng(n)
    queue = rng.integers(0, 240, (n, 2)).astype(np.uint32)
    active = (rng.random(n) < 0.3).astype(np.uint32) * rng.integers(1, 3, n).astype(np.uint32)   # (any non-zero word is a set flag)
    if n > 5:
        active[:3] = 1; active[-2:] = 1
    out_xy = np.full((max(n, 1), 2), 0xFFFFFFFF, np.uint32)
    out_q = np.full(max(n, 1), 0xFFFFFFFF, np.uint32)
    count = np.full(1, 0xFFFFFFFF, np.uint32)
    q = np.ascontiguousarray(queue)
    assert noise.emu_noise_compact(q.ctypes.data, active.ctypes.data, n, out_xy.ctypes.data, out_q.ctypes.data, count.ctypes.data) == 0
    keep = np.flatnonzero(active)
    assert int(count[0]) == len(keep)
    assert (out_q[:len(keep)] == keep).all()
    assert (out_xy[:len(keep)] == queue[keep]).all()
    assert (out_q[len(keep):] == 0xFFFFFFFF).all()   # nothing written past the count


# ---- range launches over the list of active tiles, against the oracle's film of exactly those tiles' samples

W, H = 32, 16   # 8 tiles; every third: queue entries 0, 3 and 6
SCATTER = slice(0, None, 3)
LIST_RANGES = [(4, 8), (8, 16)]   # a round's even and odd halves (min_spp 8 of a 16-sample frame, round 1)


@pytest.fixture(scope="module")
def cornell_list(tmp_path_factory, built):
    d = str(tmp_path_factory.mktemp("noise_list"))
    scenes.write_assets(d)
    p = os.path.join(d, "cornell.json")
    with open(p, "w") as f:
        json.dump(scenes.cornell_box(W, H, R.SPP), f)
    scene, *_ = T.Scene.load_file(p)
    flat = scene.flatten(0)
    q = R.tile_queue(W, H)[SCATTER]
    return scene, flat, q, {rng: R.oracle_range(flat, q, rng) for rng in LIST_RANGES}


@pytest.fixture(scope="module")
def flag_list(tmp_path_factory, built):
    d = str(tmp_path_factory.mktemp("noise_flag"))
    path = scenes.write_waving_flag(d, grid=6, n_keys=3, width=W, height=H, samples=R.SPP, frames=4, scene_time=2.0)
    scene, *_ = T.Scene.load_file(path)
    flat = scene.flatten(1)
    q = R.tile_queue(W, H)[SCATTER]
    return scene, flat, q, {rng: R.oracle_range(flat, q, rng) for rng in LIST_RANGES}


LIST_CASES = [("tiles", {"film_rows": -1}, {}), ("tiles", {"film_rows": -1}, {"TRAYHIP_TILE_SLICES": "3"}), ("wavefront", {}, {}),
              ("wavefront", {}, {"TRAYHIP_WF_SLICES": "4"})]


@pytest.mark.parametrize("case", LIST_CASES, ids=["tiles", "tiles-3-slices", "wavefront", "wavefront-4-slices"])
def test_range_launches_over_a_scattered_tile_list(case, cornell_list, emu_ranges, monkeypatch):
    kind, kw, env = case
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    _, flat, q, refs = cornell_list
    assert len(q) == 3 and not (np.diff(np.arange(8)[SCATTER]) == 1).any()
    for rng in LIST_RANGES:
        img, counts = EF.render_range(emu_ranges, kind, flat, q, rng, **kw)
        ref, ref_counts = refs[rng]
        assert counts == ref_counts and counts[0] == len(q) * 64 * (rng[1] - rng[0]), (rng, counts, ref_counts)
        R.assert_film_matches(img, ref, f"{kind} {env} list {q.tolist()} range {rng}")


def test_sampler_pass_over_a_scattered_tile_list(flag_list, emu_ranges):
    _, flat, q, refs = flag_list
    for rng in LIST_RANGES:
        img, counts = EF.render_range(emu_ranges, "sampler", flat, q, rng)
        ref, ref_counts = refs[rng]
        assert counts == ref_counts, (rng, counts, ref_counts)
        R.assert_film_matches(img, ref, f"sampler pass list {q.tolist()} range {rng}")

