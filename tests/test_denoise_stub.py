"""tray_denoise_device through the real library against the stand-in runtime (tests/stubs/fakehip.c: one log line per launch of
libtrayhip_denoise.so), as tests/test_noise_target_stub.py: every TRAY_E_INVALID case of include/trayhip.h,
tray_denoise_scratch_bytes, the three launches of a call on the caller's stream (k_dn_prepare<0>, k_dn_prepare<1>, k_dn_filter<patch> over the
32 x 16 tiles), and tray_render_tiles_device / tray_render_noise_target_device launching what they launched before."""
import os

from _stub import events, stub   # (stub: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r'''
import ctypes as C, os, sys
sys.path.insert(0, %(root)r)
import tray_rust_amd as T
from tray_rust_amd import _lib as L, scenes
lib = T.lib()
mode = %(mode)r
W, H = 70, 40
nb = lib.tray_denoise_scratch_bytes(W, H)
print("SCRATCH", nb)
bufs = [C.create_string_buffer(W * H * 16 + 16) for _ in range(3)]
scr = C.create_string_buffer(int(nb) + 16)
al = lambda b: (C.addressof(b) + 15) & ~15
even, odd, out, scratch = al(bufs[0]), al(bufs[1]), al(bufs[2]), al(scr)
def call(w=W, h=H, e=even, o=odd, r=7, f=3, k=0.45, out_=out, s=scratch, stream=None):
    return lib.tray_denoise_device(w, h, e, o, r, f, k, out_, s, stream)
if mode == "errors":
    print("CASE init", lib.tray_init(0))
    for name, kw in [("w0", dict(w=0)), ("h0", dict(h=0)), ("r0", dict(r=0)), ("r11", dict(r=11)), ("f4", dict(f=4)), ("k0", dict(k=0.0)),
                     ("kneg", dict(k=-0.45)), ("knan", dict(k=float("nan"))), ("kinf", dict(k=float("inf"))), ("null_even", dict(e=None)),
                     ("null_odd", dict(o=None)), ("null_out", dict(out_=None)), ("null_scratch", dict(s=None)), ("same_films", dict(o=even)),
                     ("out_is_even", dict(out_=even)), ("out_is_odd", dict(out_=odd)), ("misaligned", dict(e=even + 4))]:
        print("CASE", name, call(**kw))
    print("CASE smallest", call(w=1, h=1, r=1, f=0))
elif mode == "sizes":
    for w, h in [(0, 0), (0, 9), (9, 0), (1, 1), (1, 2), (2, 1), (31, 17), (32, 17), (32, 18), (1920, 1080), (65535, 65535)]:
        print("BYTES", w, h, lib.tray_denoise_scratch_bytes(w, h))
elif mode == "launches":
    T.check(lib.tray_init(0))
    stream = C.c_void_p(0x5150)   # (the stand-in runtime only records the handle)
    print("RC", call(stream=stream))
    print("RC_F1", call(w=32, h=16, r=10, f=1))
    print("RC_F0", call(w=33, h=17, r=1, f=0))
    print("RC_F2", call(w=1, h=1, r=2, f=2))
else:
    d = %(tmp)r
    scenes.write_assets(d, cornell=(64, 48, 16))
    scene, rt, spp, fi = T.Scene.load_file(os.path.join(d, "cornell_box.json"))
    dev = scene.device_scene(0, 0)
    fb = [(C.c_float * 4)() for _ in range(2)]   # (the stand-in tile kernel leaves its mark in word 0 of the film)
    fe, fo = (C.cast(b, C.c_void_p) for b in fb)
    smp, err = (C.c_uint32 * 48)(), (C.c_float * 48)()
    print("RC_PLAIN", lib.tray_render_tiles_device(dev, 0, 0, 16, 3, fe, None))
    print("RC_NT", lib.tray_render_noise_target_device(dev, 0, 0, 8, 64, 0.05, 3, fe, fo, smp, err, None))
print("DONE")
'''


def run(stub, tmp_path, mode):
    out, log = stub(DRIVER % {"root": ROOT, "tmp": str(tmp_path), "mode": mode}, tmp_path, FAKEHIP_DEVICES=1, FAKEHIP_TILE_KERNEL=1)
    assert "DONE" in out.stdout, out.stdout + out.stderr
    return out.stdout, log


def denoise_events(log):
    """the launches of libtrayhip_denoise.so in order: (kernel, template argument, grid, block, stream)"""
    return [e[1:] for e in events(log) if e[0] == "denoise"]


def test_arguments_are_checked(stub, tmp_path):
    out, log = run(stub, tmp_path, "errors")
    rc = dict(l.split()[1:] for l in out.splitlines() if l.startswith("CASE"))
    assert rc["init"] == "0"
    for name in ["w0", "h0", "r0", "r11", "f4", "k0", "kneg", "knan", "kinf", "null_even", "null_odd", "null_out", "null_scratch", "same_films",
                 "out_is_even", "out_is_odd", "misaligned"]:
        assert rc[name] == "-1", (name, out)    # TRAY_E_INVALID
    assert rc["smallest"] == "0", out
    # only the valid call launched anything: a 1 x 1 film is one block of each kernel
    ev = denoise_events(log)
    assert [e[:4] for e in ev] == [("prepare", 0, 1, 256), ("prepare", 1, 1, 256), ("filter", 0, 1, 512)], ev
    assert not any(l.startswith(("launch", "range", "noise")) for l in log)


def test_scratch_bytes_are_monotone(stub, tmp_path):
    out, _ = run(stub, tmp_path, "sizes")
    b = {(int(w), int(h)): int(n) for _, w, h, n in (l.split() for l in out.splitlines() if l.startswith("BYTES"))}
    assert b[(0, 0)] == b[(0, 9)] == b[(9, 0)] == 0
    assert b[(1, 1)] > 0
    sizes = sorted(k for k in b if k[0] and k[1])
    for w0, h0 in sizes:
        for w1, h1 in sizes:
            if w1 >= w0 and h1 >= h0:
                assert b[(w1, h1)] >= b[(w0, h0)], ((w0, h0), (w1, h1))
                if (w1, h1) != (w0, h0):
                    assert b[(w1, h1)] > b[(w0, h0)]
    assert b[(1920, 1080)] == 1920 * 1080 * 48 and b[(65535, 65535)] == 65535 * 65535 * 48   # (no 32-bit overflow)


def test_a_call_is_three_launches_on_the_callers_stream(stub, tmp_path):
    out, log = run(stub, tmp_path, "launches")
    assert "RC 0" in out and "RC_F1 0" in out and "RC_F0 0" in out and "RC_F2 0" in out, out
    ev = denoise_events(log)
    px = lambda w, h: (w * h + 255) // 256
    tiles = lambda w, h: ((w + 31) // 32) * ((h + 15) // 16)
    assert [e[:4] for e in ev] == [
        ("prepare", 0, px(70, 40), 256), ("prepare", 1, px(70, 40), 256), ("filter", 3, tiles(70, 40), 512),
        ("prepare", 0, px(32, 16), 256), ("prepare", 1, px(32, 16), 256), ("filter", 1, 1, 512),
        ("prepare", 0, px(33, 17), 256), ("prepare", 1, px(33, 17), 256), ("filter", 0, 4, 512),
        ("prepare", 0, 1, 256), ("prepare", 1, 1, 256), ("filter", 2, 1, 512)], ev
    assert all(e[4] == "0x5150" for e in ev[:3]), ev[:3]
    assert all(e[4] in ("(nil)", "0", "0x0") for e in ev[3:]), ev[3:]
    assert not any(l.startswith(("launch", "range", "noise")) for l in log)   # nothing else was launched


def test_renders_launch_what_they_launched_before(stub, tmp_path):
    out, log = run(stub, tmp_path, "renders")
    assert "RC_PLAIN 0" in out and "RC_NT 0" in out, out
    assert denoise_events(log) == []
    assert [e for e in events(log) if e[0] in ("range", "noise")] == [
        ("range", 0, 0, 48, 16, 48, 1),
        ("range", 0, 4, 48, 64, 48, 1), ("range", 4, 8, 48, 64, 48, 1), ("noise", "error", 12, 256), ("noise", "compact", 1, 1024)]
