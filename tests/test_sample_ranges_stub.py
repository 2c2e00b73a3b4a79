"""Sample ranges through the real library against the stand-in runtimes (tests/stubs/fakehip.c, which logs the range k_path_tiles
receives in front of the launch, and tests/stubs/fakerccl.c), as tests/test_multi_stub.py: the argument checks of tray_render_samples_device,
tray_multi_set_partition and tray_multi_shard_samples, the range reaching the kernel, and tray_render_frame_multi under
TRAY_PARTITION_SAMPLES -- every device renders every tile with its own range, the ranges tile [0, spp), one grouped reduce -- while the
default partition launches what it launched before."""
import os
import re

import pytest

from _stub import stub_rccl, tile_launches as launches   # (stub_rccl: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r'''
import ctypes as C, os, sys
sys.path.insert(0, %(root)r)
import tray_rust_amd as T
from tray_rust_amd import _lib as L, multi, scenes
d = %(tmp)r
scenes.write_assets(d, cornell=(%(w)d, %(h)d, %(spp)d))
scene, rt, spp, fi = T.Scene.load_file(os.path.join(d, "cornell_box.json"))
lib = T.lib()
hip = T.Hip(device=0, seed=3)
n_dev = int(os.environ["FAKEHIP_DEVICES"])
cfg = T.Config(d, "cornell_box.json", spp, 1, fi, (0, 0))
mode = %(mode)r
if mode == "errors":
    dev = scene.device_scene(0, 0)
    film_buf = (C.c_float * 4)()   # (the stand-in kernel leaves its mark in word 0 of the film)
    film = C.cast(film_buf, C.c_void_p)
    for args in [(0, 0, 16, 5, 5), (0, 0, 16, 6, 5), (0, 0, 16, 0, 17), (0, 0, 12, 0, 4), (0, 0, 0, 0, 1)]:
        print("RANGE", *args, lib.tray_render_samples_device(dev, *args, 3, film, None))
    print("RANGE_OK", lib.tray_render_samples_device(dev, 0, 0, 16, 5, 13, 3, film, None))
    T.check(lib.tray_scene_set_sampler(dev, 1, 1, 1))
    print("UNIFORM", lib.tray_render_samples_device(dev, 0, 0, 16, 0, 8, 3, film, None))
    T.check(lib.tray_scene_set_sampler(dev, 2, 4, 16))
    print("ADAPTIVE", lib.tray_render_samples_device(dev, 0, 0, 16, 0, 8, 3, film, None))
    b, e = C.c_uint32(), C.c_uint32()
    for args in [(12, 0, 2), (16, 2, 2), (16, 0, 0)]:
        print("SHARD", *args, lib.tray_multi_shard_samples(*args, C.byref(b), C.byref(e)))
    hip.sampler = lambda dim, spp: T.sampler.Uniform(dim)
    try:
        hip.render_multi(scene, rt, cfg, list(range(n_dev)), partition="samples")
        print("MULTI_UNIFORM ok")
    except T.TrayError as err:
        print("MULTI_UNIFORM", err.code)
    print("PARTITION", lib.tray_multi_set_partition(hip._multi, 2), lib.tray_multi_set_partition(hip._multi, 1))
else:
    for world in (2, 3, 8):
        print("SHARDS", world, spp, *[multi.shard_samples(spp, r, world) for r in range(world)])
    per, ms = hip.render_multi(scene, rt, cfg, list(range(n_dev)), partition=mode)
    print("RENDER_OK", rt.pixels[0], len(per))
hip.close_multi()
print("DONE")
'''


def run(stub_rccl, tmp_path, n_dev, mode, w=64, h=48, spp=16):
    out, log = stub_rccl(DRIVER % {"root": ROOT, "tmp": str(tmp_path), "w": w, "h": h, "spp": spp, "mode": mode}, tmp_path, FAKEHIP_DEVICES=n_dev,
                         FAKEHIP_TILE_KERNEL=1)
    assert "DONE" in out.stdout, out.stdout + out.stderr
    return out.stdout, log


def test_range_arguments_are_checked_and_reach_the_kernel(stub_rccl, tmp_path):
    out, log = run(stub_rccl, tmp_path, 2, "errors")
    for args in ["0 0 16 5 5", "0 0 16 6 5", "0 0 16 0 17", "0 0 12 0 4", "0 0 0 0 1"]:   # empty, reversed, past spp, spp 12, spp 0
        assert f"RANGE {args} -1" in out, out
    assert "RANGE_OK 0" in out and "UNIFORM -4" in out and "ADAPTIVE -4" in out, out
    assert "SHARD 12 0 2 -1" in out and "SHARD 16 2 2 -1" in out and "SHARD 16 0 0 -1" in out, out
    assert "MULTI_UNIFORM -4" in out, out
    assert "PARTITION -1 0" in out, out
    (rng, launch), = launches(log)   # the one launch that was made: [5, 13) of 16, every tile of the 8 x 6 queue
    assert (rng["begin"], rng["end"]) == ("5", "13") and launch["spp"] == "16" and launch["tile_count"] == "48"
    assert sum(1 for l in log if l.startswith("nccl_reduce")) == 0   # the refused multi render started nothing


@pytest.mark.parametrize("n_dev", [2, 3, 8])
def test_samples_partition_renders_every_tile_with_one_range_per_device(stub_rccl, tmp_path, n_dev):
    spp = 16
    out, log = run(stub_rccl, tmp_path, n_dev, "samples", spp=spp)
    for world in (2, 3, 8):
        line = next(l for l in out.splitlines() if l.startswith(f"SHARDS {world} "))
        got = [tuple(int(v) for v in m) for m in re.findall(r"\((\d+), (\d+)\)", line)]
        assert got == [(r * spp // world, (r + 1) * spp // world) for r in range(world)]
    pairs = launches(log)
    assert len(pairs) == n_dev
    ranges = {}
    for rng, launch in pairs:
        ranges[int(rng["dev"])] = (int(rng["begin"]), int(rng["end"]))
        assert rng["dev"] == launch["dev"] and int(launch["tile_count"]) == 48 and int(launch["spp"]) == spp and int(launch["chunk_stride"]) == 1
    want = [(d * spp // n_dev, (d + 1) * spp // n_dev) for d in range(n_dev)]
    got = [ranges[d] for d in range(n_dev)]
    assert got == [(0, 0) if w == (0, spp) else w for w in want]   # (a whole frame is launched as the whole frame)
    if n_dev > 1:
        assert got[0][0] == 0 and got[-1][1] == spp and all(a[1] == b[0] for a, b in zip(got, got[1:]))   # no gap, no overlap
    render = next(l for l in out.splitlines() if l.startswith("RENDER_OK"))
    assert float(render.split()[1]) == n_dev * (n_dev + 1) / 2                  # every device's film joined the one sum-reduce
    assert sum(1 for l in log if l.startswith("nccl_group_start")) == 1
    assert sum(1 for l in log if l.startswith("nccl_reduce")) == n_dev


def test_devices_with_an_empty_range_launch_nothing_but_join_the_reduce(stub_rccl, tmp_path):
    out, log = run(stub_rccl, tmp_path, 8, "samples", spp=4)
    pairs = launches(log)
    assert sorted((int(r["dev"]), int(r["begin"]), int(r["end"])) for r, _ in pairs) == [(1, 0, 1), (3, 1, 2), (5, 2, 3), (7, 3, 4)]
    assert sum(1 for l in log if l.startswith("nccl_reduce")) == 8 and sum(1 for l in log if l.startswith("nccl_group_start")) == 1
    assert float(next(l for l in out.splitlines() if l.startswith("RENDER_OK")).split()[1]) == 2 + 4 + 6 + 8


@pytest.mark.parametrize("n_dev", [2, 8])
def test_default_partition_deals_tiles_as_before(stub_rccl, tmp_path, n_dev):
    """partition="tiles" (the default): the launches of tests/test_multi_stub.py -- 16-tile chunks round-robin, one launch per device that has
    tiles -- each with the whole frame (0 / 0)"""
    out, log = run(stub_rccl, tmp_path, n_dev, "tiles", spp=4)
    busy = min(n_dev, 3)   # 48 tiles = 3 chunks of 16
    pairs = launches(log)
    assert len(pairs) == busy
    assert sorted(int(l["dev"]) for _, l in pairs) == list(range(busy))
    for rng, launch in pairs:
        assert (rng["begin"], rng["end"]) == ("0", "0")
        assert int(launch["chunk"]) == 16 and int(launch["chunk_stride"]) == n_dev and int(launch["spp"]) == 4
    assert sum(int(l["tile_count"]) for _, l in pairs) == 48
    assert float(next(l for l in out.splitlines() if l.startswith("RENDER_OK")).split()[1]) == busy * (busy + 1) / 2
    assert sum(1 for l in log if l.startswith("nccl_reduce")) == n_dev
