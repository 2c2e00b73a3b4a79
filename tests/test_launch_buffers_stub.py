"""The launch buffers of a device scene -- wavefront pool, per-path transform cache, transform table -- across launches, tray_scene_set_wavefront,
tray_scene_set_transform_table and frame updates, executed in this container against the stand-in HIP runtime (tests/stubs/fakehip.c, LD_PRELOAD):
kernels do nothing, hipMemGetInfo reports FAKEHIP_FREE_BYTES, hipMalloc refuses more than FAKEHIP_MALLOC_MAX, and the wavefront schedule's
"tiles done" poll reads "all done" (FAKEHIP_WF_DONE). After every step the test reads tray_last_schedule: these are the sizes the library chose.
The expected numbers of sequences b - e were recorded from the library before its launch buffers had one owner (device_api.hip: LaunchBuffers)."""
import json
import os

import pytest

from _stub import stub   # (a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TR_XF_REC = 32   # floats per record of the cache and the table (dev_anim.h)
KEYS = ("pool_slots", "xf_cache_bytes", "xf_table_bytes", "transform_table")

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

STEPS = {
    # the round-6 review's sequence (second finding): a per-path launch leaves a cache of L lanes, tray_scene_set_wavefront frees the pool,
    # a table launch allocates a pool larger than L, the table goes off -- the next launch must not index the cache past its L lanes
    "a": ["frame(0)", "hip.set_transform_table(scene, 0)", "launch(0)", "hip.set_wavefront(scene, 131072)", "show('set_wavefront')",
          "hip.set_transform_table(scene, 1)", "launch(0)", "hip.set_transform_table(scene, 0)", "launch(0)"],
    # a sequence that renders through the table: the pool and the table's buffer are there before every new frame's first launch
    "b": ["frame(0)", "hip.set_transform_table(scene, 1)", "launch(0)", "frame(1)", "launch(1)", "frame(2)", "launch(2)"],
    # ... and one that evaluates per path: the cache and the pool are handed on
    "c": ["frame(0)", "hip.set_transform_table(scene, 0)", "launch(0)", "frame(1)", "launch(1)", "frame(2)", "launch(2)"],
    # another pool size: the buffers go at once and come back at the new size with the next launch
    "d": ["frame(0)", "hip.set_transform_table(scene, 1)", "launch(0)", "hip.set_wavefront(scene, 32768)", "show('set_wavefront')", "launch(0)",
          "hip.set_wavefront(scene, 65536)", "show('set_wavefront2')", "launch(0)", "frame(1)", "launch(1)"],
    # hipMalloc refuses the table: the launch evaluates per path, the cache halves until it fits; then hipMalloc refuses more, the pool halves, and the
    # shrunk pool stays for the next frame
    "e": ["frame(0)", "hip.set_transform_table(scene, 1)", "launch(0)", "os.environ['FAKEHIP_MALLOC_MAX'] = str(64 << 20)",
          "hip.set_wavefront(scene, 524288)", "show('set_wavefront')", "launch(0)", "frame(1)", "launch(1)"],
}
ENV = {
    "a": {"TRAYHIP_XF_CACHE_BYTES": str(4 * TR_XF_REC * 4 * 32768)},   # a cache budget of 32 768 lanes for the four moving instances
    "b": {"TRAYHIP_WF_SLOTS": "65536"},
    "c": {"TRAYHIP_WF_SLOTS": "65536"},
    "d": {},
    "e": {"FAKEHIP_MALLOC_MAX": str(1 << 30)},   # (and a 128 x 128 film: 256 tiles, a pool of up to 2^20 slots)
}

# tray_last_schedule after every step: (pool_slots, xf_cache_bytes, xf_table_bytes, transform_table)
TABLE = (1 << 24) * 5 * TR_XF_REC * 4   # the table's buffer: 2^24 time indices x (four moving instances + the camera)
EXPECTED = {
    # (the cache of 32 768 lanes is too small for the 131 072 slots of the pool the table launch left: it is allocated anew for the pool)
    "a": [("frame0", (0, 0, 0, 0)), ("launch0", (32768, 16 << 20, 0, 0)), ("set_wavefront", (0, 16 << 20, 0, 0)), ("launch0", (131072, 16 << 20, TABLE, 1)),
          ("launch0", (131072, 64 << 20, TABLE, 0))],
    "b": [("frame0", (0, 0, 0, 0)), ("launch0", (65536, 0, TABLE, 1)), ("frame1", (65536, 0, TABLE, 0)), ("launch1", (65536, 0, TABLE, 1)),
          ("frame2", (65536, 0, TABLE, 0)), ("launch2", (65536, 0, TABLE, 1))],
    "c": [("frame0", (0, 0, 0, 0)), ("launch0", (65536, 32 << 20, 0, 0)), ("frame1", (65536, 32 << 20, 0, 0)), ("launch1", (65536, 32 << 20, 0, 0)),
          ("frame2", (65536, 32 << 20, 0, 0)), ("launch2", (65536, 32 << 20, 0, 0))],
    "d": [("frame0", (0, 0, 0, 0)), ("launch0", (262144, 0, TABLE, 1)), ("set_wavefront", (0, 0, TABLE, 1)), ("launch0", (32768, 0, TABLE, 1)),
          ("set_wavefront2", (0, 0, TABLE, 1)), ("launch0", (65536, 0, TABLE, 1)), ("frame1", (65536, 0, TABLE, 0)), ("launch1", (65536, 0, TABLE, 1))],
    "e": [("frame0", (0, 0, 0, 0)), ("launch0", (1 << 20, 512 << 20, 0, 0)), ("set_wavefront", (0, 512 << 20, 0, 0)), ("launch0", (131072, 512 << 20, 0, 0)),
          ("frame1", (131072, 512 << 20, 0, 0)), ("launch1", (131072, 512 << 20, 0, 0))],
}


def run(stub, tmp_path, seq):
    env = dict(FAKEHIP_DEVICES=1, FAKEHIP_WF_DONE=1, FAKEHIP_FREE_BYTES=4 << 30, TRAYHIP_MODE="wave")
    for k in ("TRAYHIP_WF_SLOTS", "TRAYHIP_XF_TABLE", "TRAYHIP_XF_CACHE_BYTES", "FAKEHIP_MALLOC_MAX", "FAKEHIP_LOG", "FAKEHIP_TILE_KERNEL"):
        env[k] = None   # (not inherited)
    env.update(ENV[seq])
    steps = "\n".join("    " + s for s in STEPS[seq])
    out, _ = stub(DRIVER % {"root": ROOT, "tmp": str(tmp_path), "size": 128 if seq == "e" else 64, "steps": steps}, tmp_path, **env)
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
