"""Sample ranges on the GPU (tray_render_samples_device, Hip.render_progressive, render_multi(partition="samples")): the films of ranges
that partition [0, spp) add up to tray_render_tiles_device's film (2e-5 of the image's largest value: the order of the f32 sums) and to the
oracle's frame (RMSE < 1e-4), a range renders exactly its samples (TrayKernelTiming.samples, and on a small image the oracle's film of those
samples), on every schedule: the tile kernel, the wavefront schedule, the moving box with the transform table and with per-path evaluation,
an AnimatedMesh through the sampler pass, and Whitted."""
import json
import os

import numpy as np
import pytest

import tray_rust_amd as T
from tray_rust_amd import scenes
import _oracle as O

pytestmark = pytest.mark.gpu
PARTITION_16 = [(0, 5), (5, 13), (13, 16)]


def rgb(img):
    return img[..., :3] / np.maximum(img[..., 3:], 1e-20)


def rmse(a, b):
    return float(np.sqrt(np.mean((rgb(a) - rgb(b)) ** 2)))


def config(fi, frame, spp):
    c = T.Config(".", "s", spp, 1, fi, (0, 0))
    c.current_frame = frame
    return c


def device_film(scene, hip, frame, spp, rng=None):
    """one launch into a zeroed device film: the samples rng of every tile (rng None: tray_render_tiles_device); returns (film, timing)"""
    import torch
    w, h = scene.flatten(frame).contents.film.width, scene.flatten(frame).contents.film.height
    film = torch.zeros(w * h * 4, dtype=torch.float32, device="cuda:0")
    if rng is None:
        hip.render_device(scene, frame, (0, 0), spp, film.data_ptr())
    else:
        hip.render_samples_device(scene, frame, (0, 0), spp, rng, film.data_ptr())
    torch.cuda.synchronize()
    return film.cpu().numpy().reshape(h, w, 4), hip.timing(scene)


def check_partition(scene, frame, spp, parts, seed, what, hip_setup=None):
    hip = T.Hip(0, seed=seed)
    if hip_setup:
        scene.device_scene(frame, 0)
        hip_setup(hip, scene)
    n_tiles = len(T.BlockQueue((scene.flatten(frame).contents.film.width, scene.flatten(frame).contents.film.height), (8, 8)))
    total = None
    for rng in parts:
        img, tim = device_film(scene, hip, frame, spp, rng)
        assert tim.samples == 64 * n_tiles * (rng[1] - rng[0]), (what, rng, tim.samples)
        total = img if total is None else total + img
    full, tim = device_film(scene, hip, frame, spp)
    assert tim.samples == 64 * n_tiles * spp
    scale = max(1.0, float(np.abs(full).max()))
    d = float(np.abs(total - full).max())
    print(f"{what}: sum of {parts} against the whole frame: max difference {d:.2e} (bar {2e-5 * scale:.2e})")
    assert d <= 2e-5 * scale, what
    cpu, _ = O.render_tiles(scene.flatten(frame), spp, seed=seed)
    r = rmse(total, cpu)
    print(f"{what}: RMSE against the oracle {r:.3e}")
    assert r < 1e-4, what
    return hip


def load(d, tmp_path, name="s.json"):
    scenes.write_assets(str(tmp_path))
    p = os.path.join(str(tmp_path), name)
    with open(p, "w") as f:
        json.dump(d, f)
    return T.Scene.load_file(p)


@pytest.mark.parametrize("name", ["cornell_box", "smallpt"])
def test_tile_kernel_ranges_add_up(name, tmp_path):
    scene, _, _, fi = load(getattr(scenes, name)(64, 64, 16), tmp_path)
    check_partition(scene, 0, 16, PARTITION_16, 3, f"{name} tile kernel")
    check_partition(scene, 0, 64, [(0, 3), (3, 50), (50, 64)], 3, f"{name} tile kernel, 64 spp")


def test_wavefront_ranges_add_up(tmp_path, monkeypatch):
    monkeypatch.setenv("TRAYHIP_MODE", "wave")
    scene, _, _, fi = load(scenes.cornell_box(64, 64, 16), tmp_path)
    check_partition(scene, 0, 16, PARTITION_16, 3, "cornell_box TRAYHIP_MODE=wave")
    monkeypatch.setenv("TRAYHIP_WF_SLICES", "4")
    scene.release_device()
    check_partition(scene, 0, 64, [(0, 3), (3, 50), (50, 64)], 3, "cornell_box TRAYHIP_MODE=wave, 4 slices")


def test_tr15_stand_in_ranges_add_up(tmp_path):
    """59 instances: the wavefront schedule by default"""
    p, _ = scenes.write_tr15_like_assets(str(tmp_path), film=(64, 48, 256), detail=0.05)
    scene, _, _, fi = T.Scene.load_file(p)
    hip = check_partition(scene, 330, 256, [(0, 3), (3, 150), (150, 256)], 2, "tr15_like")
    assert hip.schedule(scene)["launched_wavefront"] == 1


@pytest.mark.parametrize("table", [1, 0], ids=["table", "per-path"])
def test_moving_box_ranges_add_up(table, tmp_path):
    scene, _, _, fi = T.Scene.load_file(scenes.write_moving_box(str(tmp_path), width=64, height=64, samples=32))
    check_partition(scene, 0, 32, [(0, 5), (5, 13), (13, 32)], 9, f"moving_box, transform table {table}",
                    hip_setup=lambda hip, sc: hip.set_transform_table(sc, table))


def test_animated_mesh_ranges_through_the_sampler_pass(tmp_path):
    path = scenes.write_waving_flag(str(tmp_path), grid=6, n_keys=3, width=64, height=64, samples=16, frames=4, scene_time=2.0)
    scene, *_ = T.Scene.load_file(path)
    check_partition(scene, 1, 16, PARTITION_16, 2, "waving_flag (k_sampler_pass)")


def test_whitted_ranges_add_up(tmp_path):
    d = scenes.smallpt(64, 64, 16)
    d["integrator"] = {"type": "whitted", "min_depth": 4}
    scene, *_ = load(d, tmp_path)
    check_partition(scene, 0, 16, PARTITION_16, 3, "smallpt Whitted")


def test_each_range_is_the_oracle_film_of_its_samples(tmp_path):
    """16 x 16 pixels: every range's film against the oracle's RenderTarget::write of exactly its samples"""
    scene, *_ = load(scenes.cornell_box(16, 16, 16), tmp_path)
    flat = scene.flatten(0)
    hip = T.Hip(0, seed=7)
    q = np.array(T.BlockQueue((16, 16), (8, 8)).blocks, np.uint32).reshape(-1, 2)
    r = 6
    for rng in PARTITION_16 + [(7, 8)]:
        img, tim = device_film(scene, hip, 0, 16, rng)
        ref = np.zeros((16 + 2 * r, 16 + 2 * r, 4), np.float32)
        n_vert = 0
        for tile in q:
            px, py = np.meshgrid(np.arange(8) + 8 * int(tile[0]), np.arange(8) + 8 * int(tile[1]))
            n = rng[1] - rng[0]
            out = O.sample_radiance(flat, np.repeat(px.ravel(), n), np.repeat(py.ravel(), n), np.tile(np.arange(*rng), 64), 16, seed=7)
            n_vert += int(out[:, 5].sum())
            patches = O.film_patches(flat.contents.film, (int(tile[0]), int(tile[1])), np.concatenate([out[:, 3:5], out[:, 0:3]], 1), r)
            for (x, y), p in zip(np.floor(out[:, 3:5]).astype(int), patches):
                ref[y:y + 2 * r + 1, x:x + 2 * r + 1] += p
        ref = ref[r:r + 16, r:r + 16]
        assert tim.samples == 64 * len(q) * (rng[1] - rng[0])
        assert abs(int(tim.vertices) - n_vert) <= 1e-3 * n_vert
        t_img, t_ref = img[..., 3] != 0, ref[..., 3] != 0
        assert (t_img == t_ref).all(), rng
        wr = np.abs(img[..., 3] - ref[..., 3])[t_ref] / ref[..., 3][t_ref]
        assert wr.max() <= 2e-5, (rng, wr.max())
        assert rmse(img, ref) < 1e-4, rng


def test_progressive_passes_end_at_the_frame(tmp_path):
    scene, rt, _, fi = load(scenes.cornell_box(64, 64, 16), tmp_path)
    hip = T.Hip(0, seed=5)
    cfg = config(fi, 0, 16)
    hip.render(scene, rt, cfg)
    want = rt.get_renderf32().reshape(64, 64, 4).copy()
    rt.clear()
    done = []
    for k, (n, r) in enumerate(hip.render_progressive(scene, rt, cfg, 3)):
        done.append(n)
        img = r.get_renderf32().reshape(64, 64, 4)
        if k == 0:
            assert (img[..., 3] > 0).all()
    assert done == [5, 10, 16]
    got = rt.get_renderf32().reshape(64, 64, 4)
    assert np.abs(got - want).max() <= 2e-5 * max(1.0, float(np.abs(want).max()))


def test_samples_partitioned_multi_gpu_matches_tiles(tmp_path):
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs 2 GPUs")
    scene, rt, _, fi = load(scenes.cornell_box(64, 64, 16), tmp_path)
    hip = T.Hip(0, seed=5)
    cfg = config(fi, 0, 16)
    hip.render_multi(scene, rt, cfg, [0, 1], partition="tiles")
    tiles = rt.get_renderf32().reshape(64, 64, 4).copy()
    rt.clear()
    per, _ = hip.render_multi(scene, rt, cfg, [0, 1], partition="samples")
    got = rt.get_renderf32().reshape(64, 64, 4)
    assert [p.samples for p in per] == [64 * 64 * 8, 64 * 64 * 8]
    assert np.abs(got - tiles).max() <= 2e-5 * max(1.0, float(np.abs(tiles).max()))
    hip.close_multi()
