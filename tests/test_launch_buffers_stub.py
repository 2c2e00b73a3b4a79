"""The launch buffers of a device scene -- wavefront pool, per-path transform cache, transform table -- across launches, tray_scene_set_wavefront,
tray_scene_set_transform_table and frame updates, executed in this container against the stand-in HIP runtime (tests/stubs/fakehip.c, LD_PRELOAD):
kernels do nothing, hipMemGetInfo reports FAKEHIP_FREE_BYTES, hipMalloc refuses more than FAKEHIP_MALLOC_MAX, and the wavefront schedule's
"tiles done" poll reads "all done" (FAKEHIP_WF_DONE). After every step the test reads tray_last_schedule: these are the sizes the library chose.
The expected numbers of sequences b - e were recorded from the library before its launch buffers had one owner (device_api.hip: LaunchBuffers)."""
import json
import os

import pytest

from _launch_buffer_sequences import ENV, EXPECTED, FREE_BYTES, KEYS, STEPS, TR_XF_REC, film_size
from _stub import stub   # (a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r'''
import json, os, sys
sys.path.insert(0, %(root)r)
import tray_rust_amd as T
from tray_rust_amd import scenes
scene, rt, _, fi = T.Scene.load_file(scenes.write_moving_box(%(tmp)r, width=%(size)d, height=%(size)d, samples=16))
hip = T.Hip(0, seed=4)

def config(frame):
    c = T.Config(".", "s", 16, 1, fi, (0, 0))
    c.current_frame = frame
    return c

def show(label):
    print("STEP", label, json.dumps(hip.schedule(scene)), flush=True)

def frame(f):   # tray_scene_update_frame (or tray_scene_create), then the state before the frame's first launch
    scene.device_scene(f, 0)
    show("frame%%d" %% f)

def launch(f):
    rt.clear()
    hip.render(scene, rt, config(f))
    show("launch%%d" %% f)

try:
%(steps)s
    print("DONE")
except T.TrayError as e:
    print("TRAY_ERROR", e.code, e.message)
'''


def run(stub, tmp_path, seq):
    env = dict(FAKEHIP_DEVICES=1, FAKEHIP_WF_DONE=1, FAKEHIP_FREE_BYTES=FREE_BYTES, TRAYHIP_MODE="wave")
    for k in ("TRAYHIP_WF_SLOTS", "TRAYHIP_XF_TABLE", "TRAYHIP_XF_CACHE_BYTES", "FAKEHIP_MALLOC_MAX", "FAKEHIP_LOG", "FAKEHIP_TILE_KERNEL"):
        env[k] = None   # (not inherited)
    env.update(ENV[seq])
    steps = "\n".join("    " + s for s in STEPS[seq])
    out, _ = stub(DRIVER % {"root": ROOT, "tmp": str(tmp_path), "size": film_size(seq), "steps": steps}, tmp_path, **env)
    assert "DONE" in out.stdout, out.stdout + out.stderr
    return [(l.split()[1], json.loads(l.split(None, 2)[2])) for l in out.stdout.splitlines() if l.startswith("STEP")]


def numbers(steps):
    return [(label, tuple(sch[k] for k in KEYS)) for label, sch in steps]


@pytest.mark.parametrize("seq", sorted(STEPS))
def test_launch_buffers_through_the_abi(stub, tmp_path, seq, built):
    steps = run(stub, tmp_path, seq)
    for label, sch in steps:
        # the bound that keeps the stage kernels inside the per-path cache: a wavefront launch that evaluates per path has a cache for every pool slot
        if sch["launched_wavefront"] and not sch["transform_table"]:
            assert sch["xf_cache_bytes"] >= sch["pool_slots"] * sch["n_moving"] * TR_XF_REC * 4, (seq, label, sch)
    assert numbers(steps) == EXPECTED[seq]
