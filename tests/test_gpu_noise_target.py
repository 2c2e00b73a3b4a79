"""Rendering to a noise threshold on the GPU (tray_render_noise_target_device, Hip.render_noise_target).

At threshold 0 every tile takes max_spp and even + odd is tray_render_tiles_device's film (2e-5 of the image's largest value: the order of the
f32 sums), on every schedule: the tile kernel, the wavefront schedule of the >16-instance stand-in, the moving box with the transform table and
with per-path evaluation, an AnimatedMesh through the sampler pass, and Whitted. At a huge threshold every tile stops at min_spp with the film of
[0, min_spp). In a frame that is partly background, the background tiles stop at min_spp with error 0 while lit tiles go on. On a small image
with a real threshold the film is the oracle's film of exactly each tile's [0, n_t), and the reported errors are the header's metric of the
returned films."""
import ctypes as C

import numpy as np
import pytest

import tray_rust_amd as T
from tray_rust_amd import scenes
from _noise_ref import (assert_close, assert_ulps, device_film, load, numpy_tile_error, oracle_film, pixels_in_image, queue, rmse, size,
                        spheres_in_the_dark)

pytestmark = pytest.mark.gpu


def noise_target(scene, hip, frame, min_spp, max_spp, threshold):
    """one tray_render_noise_target_device call over the whole queue; returns (even, odd, tile_samples, tile_error, timing)"""
    import torch
    w, h = size(scene, frame)
    dev = scene.device_scene(frame, 0)
    spp = hip._select_sampler(dev, max_spp)
    even = torch.zeros(w * h * 4, dtype=torch.float32, device="cuda:0")
    odd = torch.zeros_like(even)
    torch.cuda.synchronize()
    n = len(queue(scene, frame))
    smp, err = np.zeros(n, np.uint32), np.zeros(n, np.float32)
    T.check(T.lib().tray_render_noise_target_device(dev, 0, 0, min_spp, spp, float(threshold), hip.seed, C.c_void_p(even.data_ptr()),
                                                    C.c_void_p(odd.data_ptr()), smp.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                    err.ctypes.data_as(C.POINTER(C.c_float)), None))
    torch.cuda.synchronize()
    return even.cpu().numpy().reshape(h, w, 4), odd.cpu().numpy().reshape(h, w, 4), smp, err, hip.timing(scene)


def check_threshold_zero(scene, frame, min_spp, max_spp, seed, what, hip_setup=None):
    hip = T.Hip(0, seed=seed)
    if hip_setup:
        scene.device_scene(frame, 0)
        hip_setup(hip, scene)
    even, odd, smp, err, tim = noise_target(scene, hip, frame, min_spp, max_spp, 0.0)
    q = queue(scene, frame)
    assert (smp == max_spp).all(), (what, np.unique(smp))
    assert tim.samples == int((pixels_in_image(scene, frame, q) * max_spp).sum()), (what, tim.samples)
    rounds = int(np.log2(max_spp // min_spp)) + 1
    assert tim.launches >= 4 * rounds, (what, tim.launches)
    full = device_film(scene, hip, frame, max_spp)
    assert_close(even + odd, full, f"{what}: even + odd against tray_render_tiles_device")
    return hip


def test_threshold_zero_tile_kernel(tmp_path):
    scene, *_ = load(scenes.cornell_box(64, 64, 32), tmp_path)
    hip = check_threshold_zero(scene, 0, 4, 32, 3, "cornell_box tile kernel")
    assert hip.schedule(scene)["launched_wavefront"] == 0


def test_threshold_zero_wavefront(tmp_path):
    """59 instances: the wavefront schedule by default"""
    p, _ = scenes.write_tr15_like_assets(str(tmp_path), film=(64, 48, 64), detail=0.05)
    scene, *_ = T.Scene.load_file(p)
    hip = check_threshold_zero(scene, 330, 8, 64, 2, "tr15_like wavefront")
    assert hip.schedule(scene)["launched_wavefront"] == 1


@pytest.mark.parametrize("table", [1, 0], ids=["table", "per-path"])
def test_threshold_zero_moving_box(table, tmp_path):
    scene, *_ = T.Scene.load_file(scenes.write_moving_box(str(tmp_path), width=64, height=64, samples=32))
    check_threshold_zero(scene, 0, 4, 32, 9, f"moving_box, transform table {table}", hip_setup=lambda hip, sc: hip.set_transform_table(sc, table))


def test_threshold_zero_animated_mesh_sampler_pass(tmp_path):
    path = scenes.write_waving_flag(str(tmp_path), grid=6, n_keys=3, width=64, height=64, samples=16, frames=4, scene_time=2.0)
    scene, *_ = T.Scene.load_file(path)
    check_threshold_zero(scene, 1, 2, 16, 2, "waving_flag (k_sampler_pass)")


def test_threshold_zero_whitted(tmp_path):
    d = scenes.smallpt(64, 64, 16)
    d["integrator"] = {"type": "whitted", "min_depth": 4}
    scene, *_ = load(d, tmp_path)
    check_threshold_zero(scene, 0, 2, 16, 3, "smallpt Whitted")


def test_huge_threshold_stops_every_tile_at_min_spp(tmp_path):
    scene, *_ = load(scenes.cornell_box(64, 64, 64), tmp_path)
    hip = T.Hip(0, seed=4)
    even, odd, smp, err, tim = noise_target(scene, hip, 0, 8, 64, 3.0e38)
    assert (smp == 8).all() and np.isfinite(err).all() and (err < 3.0e38).all()
    assert tim.samples == 64 * 64 * 8 and tim.launches == 4
    assert_close(even + odd, device_film(scene, hip, 0, 64, (0, 8)), "huge threshold against [0, 8)")
    assert_close(even, device_film(scene, hip, 0, 64, (0, 4)), "even film against [0, 4)")


def test_background_tiles_stop_at_min_spp(tmp_path):
    """tiles farther than the filter radius from any geometry see radiance 0 in both films: error 0, so they stop after round 0; tiles on the
    lit spheres are noisy and take more samples"""
    scene, *_ = load(spheres_in_the_dark(64, 64, 128), tmp_path)
    hip = T.Hip(0, seed=6)
    even, odd, smp, err, tim = noise_target(scene, hip, 0, 4, 128, 0.05)
    full = device_film(scene, hip, 0, 128)
    q = queue(scene, 0)
    r = 2   # (the Mitchell filter's radius: a sample reaches 2 pixels in each direction)
    pad = np.pad(np.abs(full[..., :3]).sum(-1), r)
    dark = np.array([pad[8 * int(y):8 * int(y) + 8 + 2 * r, 8 * int(x):8 * int(x) + 8 + 2 * r].max() == 0.0 for x, y in q])
    print(f"{dark.sum()} of {len(q)} tiles see only background; samples per tile: {np.unique(smp, return_counts=True)}")
    assert dark.sum() >= 4 and (~dark).sum() >= 4
    assert (smp[dark] == 4).all() and (err[dark] == 0.0).all()
    assert (smp[~dark] > 4).any()
    assert tim.samples == int((64 * smp.astype(np.int64)).sum())
    # every lit tile that stopped early did so below the threshold
    assert (err[smp < 128] < 0.05).all()


@pytest.mark.parametrize("dims", [(16, 16), (24, 16)], ids=["16x16", "24x16"])
def test_small_image_is_the_oracle_film_of_each_tiles_prefix(dims, tmp_path):
    w, h = dims
    scene, *_ = load(scenes.cornell_box(w, h, 64), tmp_path)
    flat = scene.flatten(0)
    hip = T.Hip(0, seed=7)
    lo, hi, thr = 2, 64, 0.35
    even, odd, smp, err, tim = noise_target(scene, hip, 0, lo, hi, thr)
    q = queue(scene, 0)
    print(f"{w}x{h}: samples per tile {smp.tolist()}, errors {err.tolist()}")
    assert all(lo <= n <= hi and (n & (n - 1)) == 0 for n in smp)
    assert (err[smp < hi] < thr).all()
    assert tim.samples == int((64 * smp.astype(np.int64)).sum())
    img = even + odd
    ref = oracle_film(flat, q, smp, hi, 7)
    t_img, t_ref = img[..., 3] != 0, ref[..., 3] != 0
    assert (t_img == t_ref).all()
    wr = np.abs(img[..., 3] - ref[..., 3])[t_ref] / ref[..., 3][t_ref]
    assert wr.max() <= 2e-5, wr.max()
    assert rmse(img, ref) < 1e-4
    # a tile's error is taken in the round it stops; later rounds of its neighbours still splat into its edge pixels (the filter's footprint),
    # so it is the metric of the returned films where no neighbour took more samples -- every tile that took max_spp among them
    n_of = {(int(x), int(y)): int(n) for (x, y), n in zip(q, smp)}
    final = np.array([all(n_of.get((int(x) + dx, int(y) + dy), 0) <= n for dx in (-1, 0, 1) for dy in (-1, 0, 1)) for (x, y), n in zip(q, smp)])
    assert final[smp == smp.max()].all()
    assert_ulps(err[final], np.array([numpy_tile_error(even, odd, t) for t in q[final]], np.float32), 4, f"{w}x{h} tile errors")


def test_python_render_noise_target(tmp_path):
    scene, rt, _, fi = load(scenes.cornell_box(64, 64, 32), tmp_path)
    hip = T.Hip(0, seed=5)
    cfg = T.Config(".", "s", 32, 1, fi, (0, 0))
    rt.clear()
    smp, err = hip.render_noise_target(scene, rt, cfg, 0.0, min_spp=4)
    even, odd, smp_c, err_c, _ = noise_target(scene, T.Hip(0, seed=5), 0, 4, 32, 0.0)
    assert smp.dtype == np.uint32 and err.dtype == np.float32 and len(smp) == len(queue(scene, 0))
    assert (smp == smp_c).all() and (smp == 32).all()
    np.testing.assert_allclose(err, err_c, rtol=1e-3)
    assert_close(rt.get_renderf32().reshape(64, 64, 4), even + odd, "render_noise_target's film against the C call's")
