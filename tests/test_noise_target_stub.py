"""tray_render_noise_target_device through the real library against the stand-in runtime (tests/stubs/fakehip.c: a log line of the
sample range every tile kernel receives and one of every launch of libtrayhip_noise.so), as tests/test_sample_ranges_stub.py: the
argument checks, round 0's two range launches over the whole tile range followed by the error and compaction kernels, and a plain
tray_render_tiles_device that launches what it launched before. The stand-in kernels do nothing, so the compacted list is empty after round 0
and the call ends there."""
import os

from _stub import events, stub   # (stub: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r'''
import ctypes as C, os, sys
sys.path.insert(0, %(root)r)
import tray_rust_amd as T
from tray_rust_amd import _lib as L, scenes
d = %(tmp)r
scenes.write_assets(d, cornell=(64, 48, 16))
scene, rt, spp, fi = T.Scene.load_file(os.path.join(d, "cornell_box.json"))
lib = T.lib()
dev = scene.device_scene(0, 0)
bufs = [(C.c_float * 4)() for _ in range(2)]   # (the stand-in tile kernel leaves its mark in word 0 of the film)
even, odd = (C.cast(b, C.c_void_p) for b in bufs)
smp, err = (C.c_uint32 * 48)(), (C.c_float * 48)()
def call(start, count, lo, hi, thr, e=even, o=odd, s=smp, r=err):
    return lib.tray_render_noise_target_device(dev, start, count, lo, hi, thr, 3, e, o, s, r, None)
mode = %(mode)r
if mode == "errors":
    nan = float("nan")
    for name, args in [("min1", (0, 0, 1, 16, 0.1)), ("min0", (0, 0, 0, 16, 0.1)), ("min3", (0, 0, 3, 16, 0.1)), ("max12", (0, 0, 4, 12, 0.1)),
                       ("max_below_min", (0, 0, 16, 8, 0.1)), ("negative", (0, 0, 4, 16, -0.5)), ("nan", (0, 0, 4, 16, nan))]:
        print("CASE", name, call(*args))
    print("CASE null_even", call(0, 0, 4, 16, 0.1, e=None))
    print("CASE null_odd", call(0, 0, 4, 16, 0.1, o=None))
    print("CASE same_film", call(0, 0, 4, 16, 0.1, o=even))
    print("CASE null_samples", call(0, 0, 4, 16, 0.1, s=None))
    print("CASE null_error", call(0, 0, 4, 16, 0.1, r=None))
    print("CASE null_scene", lib.tray_render_noise_target_device(None, 0, 0, 4, 16, 0.1, 3, even, odd, smp, err, None))
    T.check(lib.tray_scene_set_sampler(dev, 1, 1, 1))
    print("CASE uniform", call(0, 0, 4, 16, 0.1))
    T.check(lib.tray_scene_set_sampler(dev, 2, 4, 16))
    print("CASE adaptive", call(0, 0, 4, 16, 0.1))
    T.check(lib.tray_scene_set_sampler(dev, 0, 1, 1))
    print("CASE min_equals_max", call(0, 0, 16, 16, 0.0))   # (the smallest valid call: one round, [0, 8) and [8, 16))
elif mode == "round0":
    print("RC", call(0, 0, 8, 64, 0.05))
    t = L.TrayKernelTiming()
    print("TIMING", lib.tray_last_timing(dev, C.byref(t)), t.launches)
    print("RC_SUB", call(5, 10, 2, 4, 0.05))
else:
    print("RC", lib.tray_render_tiles_device(dev, 0, 0, 16, 3, even, None))
print("DONE")
'''


def run(stub, tmp_path, mode):
    out, log = stub(DRIVER % {"root": ROOT, "tmp": str(tmp_path), "mode": mode}, tmp_path, FAKEHIP_DEVICES=1, FAKEHIP_TILE_KERNEL=1)
    assert "DONE" in out.stdout, out.stdout + out.stderr
    return out.stdout, log


def test_arguments_are_checked(stub, tmp_path):
    out, log = run(stub, tmp_path, "errors")
    rc = dict(l.split()[1:] for l in out.splitlines() if l.startswith("CASE"))
    for name in ["min1", "min0", "min3", "max12", "max_below_min", "negative", "nan", "null_even", "null_odd", "same_film", "null_samples",
                 "null_error", "null_scene"]:
        assert rc[name] == "-1", (name, out)    # TRAY_E_INVALID
    assert rc["uniform"] == "-4" and rc["adaptive"] == "-4", out   # TRAY_E_UNSUPPORTED
    assert rc["min_equals_max"] == "0", out
    # only the valid call launched anything: [0, 8) and [8, 16) of the 16-sample frame over the 48 tiles, the error kernel, the compaction
    assert events(log) == [("range", 0, 8, 48, 16, 48, 1), ("range", 8, 16, 48, 16, 48, 1), ("noise", "error", 12, 256), ("noise", "compact", 1, 1024)]


def test_round_zero_renders_both_halves_of_min_spp_over_the_tile_range(stub, tmp_path):
    out, log = run(stub, tmp_path, "round0")
    assert "RC 0" in out and "RC_SUB 0" in out, out
    assert "TIMING 0 4" in out, out   # two tile kernels, the error kernel and the compaction
    assert events(log) == [
        ("range", 0, 4, 48, 64, 48, 1), ("range", 4, 8, 48, 64, 48, 1), ("noise", "error", 12, 256), ("noise", "compact", 1, 1024),
        # tiles [5, 15) with min_spp 2 of a 4-sample frame
        ("range", 0, 1, 10, 4, 10, 1), ("range", 1, 2, 10, 4, 10, 1), ("noise", "error", 3, 256), ("noise", "compact", 1, 1024)]


def test_plain_render_launches_what_it_launched_before(stub, tmp_path):
    out, log = run(stub, tmp_path, "plain")
    assert "RC 0" in out, out
    assert events(log) == [("range", 0, 0, 48, 16, 48, 1)]
