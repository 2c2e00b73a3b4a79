"""tray_denoise_temporal_device and Hip.render_sequence_denoised through the real library against the stand-in runtime (tests/stubs/fakehip.c), as
tests/test_denoise_stub.py: every TRAY_E_INVALID case of include/trayhip.h with its tray_last_error text, the scratch size, the 3 (N + 1)
launches of a call on the caller's stream -- per frame k_dn_prepare<0>, k_dn_prepare<1> (logged as libtrayhip_denoise.so's) and one k_tdn_pass
over the 32 x 16 tiles (libtrayhip_temporal.so has no branch in the stand-in runtime: a plain launch line of 512 threads) --, tray_denoise_device
launching what it launched before, and the renders and passes of a four-frame sequence. The runs are made without FAKEHIP_TILE_KERNEL, which
would read a pass's arguments as the tile kernel's; render launches are told from passes by their block size (_temporal_ref.launches)."""
import os

from _stub import stub   # (a fixture)
from _temporal_ref import launches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r'''
import ctypes as C, os, sys
sys.path.insert(0, %(root)r)
sys.path.insert(0, os.path.join(%(root)r, "tests"))
import numpy as np
import tray_rust_amd as T
from tray_rust_amd import _lib as L, scenes
lib = T.lib()
mode = %(mode)r
W, H = 70, 40
FILM = W * H * 16
store = C.create_string_buffer(24 * (FILM + 16) + 16)
base = (C.addressof(store) + 15) & ~15
buf = lambda i: base + i * (FILM + 16)   # 16-byte aligned, pairwise different
even, odd, out = buf(0), buf(1), buf(2)
nb = [(buf(3 + 2 * j), buf(4 + 2 * j)) for j in range(9)]
nbytes = int(lib.tray_denoise_temporal_scratch_bytes(W, H))
print("SCRATCH", nbytes, lib.tray_denoise_temporal_scratch_bytes(0, 7), lib.tray_denoise_temporal_scratch_bytes(7, 0),
      lib.tray_denoise_temporal_scratch_bytes(65535, 65535))
scr = C.create_string_buffer(nbytes + 32)
scratch = (C.addressof(scr) + 15) & ~15
arr = lambda ptrs: (C.c_void_p * max(len(ptrs), 1))(*ptrs)
def call(w=W, h=H, e=even, o=odd, n=1, nbs=None, ne=0, no=0, r=7, rt=3, f=3, k=0.45, out_=out, s=scratch, stream=None):
    nbs = nb[:n] if nbs is None else nbs
    ne = arr([p[0] for p in nbs]) if ne == 0 else ne
    no = arr([p[1] for p in nbs]) if no == 0 else no
    return lib.tray_denoise_temporal_device(w, h, e, o, n, ne, no, r, rt, f, k, out_, s, stream)
if mode == "errors":
    print("CASE init", lib.tray_init(0))
    nan = float("nan")
    for name, kw in [("w0", dict(w=0)), ("h0", dict(h=0)), ("r0", dict(r=0, rt=0)), ("r11", dict(r=11)), ("rt0", dict(rt=0)), ("rt_above_r", dict(r=3, rt=4)),
                     ("f4", dict(f=4)), ("k0", dict(k=0.0)), ("kneg", dict(k=-0.45)), ("knan", dict(k=nan)), ("n9", dict(n=9)),
                     ("null_even", dict(e=None)), ("null_odd", dict(o=None)), ("null_out", dict(out_=None)), ("null_scratch", dict(s=None)),
                     ("null_nb_even_array", dict(ne=None)), ("null_nb_odd_array", dict(no=None)), ("null_nb_film", dict(n=2, nbs=[nb[0], (nb[1][0], None)])),
                     ("same_films", dict(o=even)), ("centre_film_twice", dict(nbs=[(even, nb[0][1])])), ("nb_film_twice", dict(n=2, nbs=[nb[0], (nb[1][0], nb[0][0])])),
                     ("out_is_even", dict(out_=even)), ("out_is_nb_film", dict(out_=nb[0][1])), ("scratch_is_nb_film", dict(s=nb[0][0])),
                     ("misaligned_even", dict(e=even + 4)), ("misaligned_nb", dict(nbs=[(nb[0][0] + 8, nb[0][1])])), ("misaligned_out", dict(out_=out + 4)),
                     ("misaligned_scratch", dict(s=scratch + 12))]:
        rc = call(**kw)
        print("CASE", name, rc, "|", lib.tray_last_error().decode())
    print("CASE smallest", call(w=1, h=1, n=0, ne=None, no=None, r=1, rt=1, f=0), "|")
elif mode == "launches":
    T.check(lib.tray_init(0))
    stream = C.c_void_p(0x5150)
    for n in (0, 1, 3):
        print("RC", n, call(n=n, stream=stream))
    print("RC_F1", call(w=33, h=17, n=2, r=3, rt=2, f=1))
    print("RC_DN", lib.tray_denoise_device(W, H, even, odd, 7, 3, 0.45, out, scratch, stream))
else:
    # Hip.render_sequence_denoised allocates its films through torch: a stand-in with host memory behind it, as the stand-in runtime's hipMalloc
    from _fake_torch import Tensor, install as fake_torch
    fake_torch()
    d = %(tmp)r
    os.makedirs(os.path.join(d, "models"), exist_ok=True)
    open(os.path.join(d, "models", "cube.obj"), "w").write(scenes.cube_obj())
    s = scenes.cornell_box(64, 48, 16)
    s["film"].update({"frames": 4, "start_frame": 0, "end_frame": 3, "scene_time": 1.0})
    scene, rt, spp, fi = T.Scene.load_file(scenes.write_scene(s, os.path.join(d, "four_frames.json")))
    hip = T.Hip(0, seed=3)
    cfg = T.Config(d, "four_frames.json", spp, 1, fi, (0, 0))
    hip.render_samples_device(scene, 0, (0, 0), 16, (0, 8), Tensor(np.zeros((48, 64, 4), np.float32)).data_ptr(), 0x5150)   # what one range launch looks like
    Tensor.count = 0
    for frame, img in hip.render_sequence_denoised(scene, cfg, range(4), reach=1):
        print("FRAME", frame, img.shape, img.dtype)
    print("FILMS", Tensor.count)
print("DONE")
'''


def run(stub, tmp_path, mode):
    out, log = stub(DRIVER % {"root": ROOT, "tmp": str(tmp_path), "mode": mode}, tmp_path, FAKEHIP_DEVICES=1, FAKEHIP_TILE_KERNEL=None, TRAYHIP_MODE=None)
    assert "DONE" in out.stdout, out.stdout + out.stderr
    return out.stdout, log


PX = lambda w, h: (w * h + 255) // 256
TILES = lambda w, h: ((w + 31) // 32) * ((h + 15) // 16)
NIL = ("(nil)", "0", "0x0")


def call_launches(w, h, n):
    """the launches of one call with n neighbours, streams cut off"""
    return [("prepare", 0, PX(w, h), 256), ("prepare", 1, PX(w, h), 256), ("pass", -1, TILES(w, h), 512)] * (n + 1)


def test_arguments_are_checked(stub, tmp_path):
    out, log = run(stub, tmp_path, "errors")
    cases = {}
    for l in out.splitlines():
        if l.startswith("CASE"):
            head, _, text = l.partition("|")
            cases[head.split()[1]] = (head.split()[2], text.strip())
    assert cases.pop("init")[0] == "0" and cases.pop("smallest")[0] == "0", out
    assert len(cases) == 28
    for name, (rc, text) in cases.items():
        assert rc == "-1", (name, rc)   # TRAY_E_INVALID
        assert text.startswith("tray_denoise_temporal_device: ") and len(text) > 35, (name, text)
    # only the valid call launched anything: a 1 x 1 film without neighbours is one block of each kernel
    assert [e[:4] for e in launches(log)] == call_launches(1, 1, 0), log


def test_scratch_bytes(stub, tmp_path):
    out, _ = run(stub, tmp_path, "launches")
    assert f"SCRATCH {70 * 40 * 128} 0 0 {65535 * 65535 * 128}" in out, out   # (no 32-bit overflow)


def test_a_call_is_three_launches_per_frame_on_the_callers_stream(stub, tmp_path):
    out, log = run(stub, tmp_path, "launches")
    for k in ("RC 0 0", "RC 1 0", "RC 3 0", "RC_F1 0", "RC_DN 0"):
        assert k in out, out
    ev = launches(log)
    want = call_launches(70, 40, 0) + call_launches(70, 40, 1) + call_launches(70, 40, 3)
    assert len(want) == 3 * (1 + 2 + 4)
    assert [e[:4] for e in ev[:len(want)]] == want, ev
    assert all(e[4] == "0x5150" for e in ev[:len(want)]), ev
    rest = ev[len(want):]
    assert [e[:4] for e in rest[:9]] == call_launches(33, 17, 2) and all(e[4] in NIL for e in rest[:9]), rest
    # tray_denoise_device on the same films: its three lines, as before
    assert [e[:4] for e in rest[9:]] == [("prepare", 0, PX(70, 40), 256), ("prepare", 1, PX(70, 40), 256), ("filter", 3, TILES(70, 40), 512)], rest
    assert all(e[4] == "0x5150" for e in rest[9:])
    assert len(log) == len(ev)   # nothing else was logged


def test_a_sequence_renders_every_frame_once_and_filters_it_with_its_neighbours(stub, tmp_path):
    out, log = run(stub, tmp_path, "sequence")
    assert [l for l in out.splitlines() if l.startswith("FRAME")] == [f"FRAME {f} (48, 64, 4) float32" for f in range(4)], out
    assert "FILMS 6" in out, out   # 2 reach + 1 pairs, rendered into again
    ev = launches(log)
    one_range, ev = ev[0], ev[1:]
    assert one_range[0] == "other"
    render = [one_range] * 2   # a frame's two range launches
    frame = lambda n: [e + ("0x5150",) for e in call_launches(64, 48, n)]
    assert ev == render * 2 + frame(1) + render + frame(2) + render + frame(2) + frame(1), ev
    assert sum(e[0] == "other" for e in ev) == 8
    assert [n // 3 for n in (len(frame(1)), len(frame(2)), len(frame(2)), len(frame(1)))] == [2, 3, 3, 2]
