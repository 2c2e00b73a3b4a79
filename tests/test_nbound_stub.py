"""tray_scene_set_noise_ratio and the two noise-target calls under it, through the real library against the stand-in runtime
(tests/stubs/fakehip.c), as tests/test_noise_target_stub.py: the setter's and the bounded calls' refusals come before any device call, ratio 0
logs exactly the launches of the call without the setter, and ratio 4 logs the launches noise_plan.h's bounded schedule predicts --
libtrayhip_nbound.so's as plain `launch` lines with their kernel symbols. The stand-in kernels do nothing, so every level list is empty after
round 0 and a call ends there: the later rounds are the emulation's to check (tests/test_nbound_emu.py)."""
import os

from _stub import events, kv, stub   # (stub: a fixture)

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
films = [(C.c_float * (64 * 48 * 4 + 4))() for _ in range(3)]
even, odd, out = (C.c_void_p((C.addressof(b) + 15) // 16 * 16) for b in films)
smp, err = (C.c_uint32 * 48)(), (C.c_float * 48)()
def call(lo, hi, thr=0.05):
    return lib.tray_render_noise_target_device(dev, 0, 0, lo, hi, thr, 3, even, odd, smp, err, None)
def launches():
    t = L.TrayKernelTiming()
    return lib.tray_last_timing(dev, C.byref(t)), t.launches
mode = %(mode)r
if mode == "refusals":
    for v in (1, 3, 6, 12, 65537, 131072, 0xffffffff):
        print("CASE set_%%d" %% v, lib.tray_scene_set_noise_ratio(dev, v))
    print("CASE set_null", lib.tray_scene_set_noise_ratio(None, 4))
    for v in (0, 2, 4, 65536):
        print("CASE ok_%%d" %% v, lib.tray_scene_set_noise_ratio(dev, v))
    T.check(lib.tray_scene_set_noise_ratio(dev, 4))
    print("CASE levels_17", call(2, 1 << 18))
    print("CASE bad_min_first", call(3, 16))
    T.check(lib.tray_scene_set_noise_ratio(dev, 0))
    print("CASE levels_17_unbounded", call(2, 1 << 18))
elif mode in ("plain", "zero"):
    if mode == "zero":
        T.check(lib.tray_scene_set_noise_ratio(dev, 4))
        T.check(lib.tray_scene_set_noise_ratio(dev, 0))
    print("RC", call(8, 64), *launches())
elif mode == "four":
    T.check(lib.tray_scene_set_noise_ratio(dev, 4))
    print("RC", call(8, 64), *launches())
    print("RC_ONE_LEVEL", call(16, 16), *launches())
elif mode == "four_filtered":
    T.check(lib.tray_scene_set_noise_ratio(dev, 4))
    n = lib.tray_noise_target_filtered_scratch_bytes(64, 48)
    scratch = (C.c_char * (n + 16))()
    sp = C.c_void_p((C.addressof(scratch) + 15) // 16 * 16)
    print("RC", lib.tray_render_noise_target_filtered_device(dev, 0, 0, 8, 64, 0.05, 3, even, odd, 7, 3, 0.45, out, sp, smp, err, None), *launches())
print("DONE")
'''


def run(stub, tmp_path, mode, tile_kernel):
    env = {"FAKEHIP_TILE_KERNEL": 1} if tile_kernel else {}
    out, log = stub(DRIVER % {"root": ROOT, "tmp": str(tmp_path), "mode": mode}, tmp_path, FAKEHIP_DEVICES=1, **env)
    assert "DONE" in out.stdout, out.stdout + out.stderr
    return out.stdout, log


def kernels(log):
    """every launch in order as (the log line's first word, the kernel's name, grid, block)"""
    names = ("k_path_tiles", "k_noise_error", "k_noise_compact", "k_nb_grid", "k_nb_pull", "k_nb_compact_level", "k_guide_mark", "k_guide_compact",
             "k_dn_filter_halves", "k_dn_filter", "k_dn_prepare")
    out = []
    for l in log:
        if l.startswith(("launch", "noise", "guide", "denoise")):
            n = kv(l)
            out.append((l.split()[0], next((k for k in names if k in n["kernel"]), n["kernel"]), int(n["grid"]), int(n["block"])))
    return out


def test_refusals_come_before_any_device_call(stub, tmp_path):
    out, log = run(stub, tmp_path, "refusals", False)
    rc = dict(l.split()[1:] for l in out.splitlines() if l.startswith("CASE"))
    for name in ["set_1", "set_3", "set_6", "set_12", "set_65537", "set_131072", "set_4294967295", "set_null", "levels_17", "bad_min_first"]:
        assert rc[name] == "-1", (name, out)   # TRAY_E_INVALID
    for name in ["ok_0", "ok_2", "ok_4", "ok_65536", "levels_17_unbounded"]:
        assert rc[name] == "0", (name, out)
    # nothing but the unbounded call at the end launched anything: its two renders, the error kernel, the compaction
    assert [k[1] for k in kernels(log)] == ["k_path_tiles", "k_path_tiles", "k_noise_error", "k_noise_compact"]


def test_ratio_zero_logs_the_launches_of_the_call_without_the_setter(stub, tmp_path):
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    plain_out, plain = run(stub, tmp_path / "a", "plain", True)
    zero_out, zero = run(stub, tmp_path / "b", "zero", True)
    assert "RC 0 0 4" in plain_out and "RC 0 0 4" in zero_out, plain_out + zero_out
    want = [("range", 0, 4, 48, 64, 48, 1), ("range", 4, 8, 48, 64, 48, 1), ("noise", "error", 12, 256), ("noise", "compact", 1, 1024)]
    assert events(plain) == want and events(zero) == want
    # ... and nothing else differs either: the same lines but for the addresses in them
    strip = lambda log: [" ".join(w for w in l.split() if "=0x" not in w) for l in log]
    assert strip(plain) == strip(zero)


def test_ratio_four_logs_the_bounded_schedule(stub, tmp_path):
    """4 levels from 8 to 64 over 48 tiles: the map, round 0's renders and error, 3 pull steps and the one level list round 0 can fill; 8 launches, as
    noise_plan.h's bound_call_launches(raw, 1 round, 1 list, 4 levels) counts. min_spp == max_spp has nothing to bound: the unbounded call."""
    out, log = run(stub, tmp_path, "four", False)
    assert "RC 0 0 8" in out and "RC_ONE_LEVEL 0 0 4" in out, out
    got = kernels(log)
    assert [k[:2] for k in got] == [("launch", "k_nb_grid"), ("launch", "k_path_tiles"), ("launch", "k_path_tiles"), ("noise", "k_noise_error")] + [
        ("launch", "k_nb_pull")] * 3 + [("launch", "k_nb_compact_level"),
        ("launch", "k_path_tiles"), ("launch", "k_path_tiles"), ("noise", "k_noise_error"), ("noise", "k_noise_compact")]
    # one thread per queue entry of the 48 tiles for the map and the pull steps, the one workgroup for the list
    assert [k[2:] for k in got if "k_nb_" in k[1]] == [(1, 256)] * 4 + [(1, 1024)]


def test_ratio_four_filtered_logs_the_bounded_schedule(stub, tmp_path):
    """the filtered rule under the bound: the first block list, the map, round 0 (renders, prepare x 2 and the halves, error), the pull steps, the level
    list, the next block list, and the final filter of the output: 2 + 1 + 6 + 3 + 1 + 2 + 3 launches"""
    out, log = run(stub, tmp_path, "four_filtered", False)
    assert "RC 0 0 18" in out, out
    assert [k[1] for k in kernels(log)] == ["k_guide_mark", "k_guide_compact", "k_nb_grid", "k_path_tiles", "k_path_tiles", "k_dn_prepare", "k_dn_prepare",
                                            "k_dn_filter_halves", "k_noise_error", "k_nb_pull", "k_nb_pull", "k_nb_pull", "k_nb_compact_level", "k_guide_mark",
                                            "k_guide_compact", "k_dn_prepare", "k_dn_prepare", "k_dn_filter"]
