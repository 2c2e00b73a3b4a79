"""tray_denoise_temporal_demodulated_device, Hip.denoise_temporal(albedos=...) and Hip.render_sequence_denoised(demodulate=True) through the real
library against the stand-in runtime (tests/stubs/fakehip.c), as tests/test_first_hit_stub.py: every TRAY_E_INVALID case of include/trayhip.h
returns before any device call -- with tests/stubs/fakehip_host_calls.c preloaded in front, which logs every wait, copy and fill --, the scratch
size, the 3 (N + 1) launches of a call in stream order with nothing between them -- per frame k_tdm_prepare, the library's own k_dn_prepare<1>
and one k_tdm_pass over the 32 x 16 tiles, all of libtrayhip_tdemod.so and therefore plain `launch` lines (a k_dn_prepare<1> of
libtrayhip_denoise.so would be logged under that library's prefix) --, the defaults of the two Python entry points launching what they launched
before, and a demodulated sequence rendering every frame's albedo film exactly once. The runs are made without FAKEHIP_TILE_KERNEL, which would
read another kernel's arguments as the tile kernel's."""
import os

import pytest

import _stub
from _stub import stub   # (a fixture)
from _tdemod_ref import launches

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
def mark(name):
    with open(os.environ["FAKEHIP_LOG"], "a") as f:
        f.write("mark name=%%s\n" %% name)
W, H = 70, 40
FILM = W * H * 16
store = C.create_string_buffer(32 * (FILM + 16) + 16)
base = (C.addressof(store) + 15) & ~15
buf = lambda i: base + i * (FILM + 16)   # 16-byte aligned, pairwise different
even, odd, alb, out = buf(0), buf(1), buf(2), buf(3)
nb = [(buf(4 + 3 * j), buf(5 + 3 * j), buf(6 + 3 * j)) for j in range(9)]
nbytes = int(lib.tray_denoise_temporal_demodulated_scratch_bytes(W, H))
print("SCRATCH", nbytes, lib.tray_denoise_temporal_demodulated_scratch_bytes(0, 7), lib.tray_denoise_temporal_demodulated_scratch_bytes(7, 0),
      lib.tray_denoise_temporal_demodulated_scratch_bytes(65535, 65535), int(lib.tray_denoise_temporal_scratch_bytes(W, H)))
scr = C.create_string_buffer(nbytes + 32)
scratch = (C.addressof(scr) + 15) & ~15
arr = lambda ptrs: (C.c_void_p * max(len(ptrs), 1))(*ptrs)
def call(w=W, h=H, e=even, o=odd, a=alb, n=1, nbs=None, ne=0, no=0, na=0, r=7, rt=3, f=3, k=0.45, out_=out, s=scratch, stream=None):
    nbs = nb[:n] if nbs is None else nbs
    ne = arr([p[0] for p in nbs]) if ne == 0 else ne
    no = arr([p[1] for p in nbs]) if no == 0 else no
    na = arr([p[2] for p in nbs]) if na == 0 else na
    return lib.tray_denoise_temporal_demodulated_device(w, h, e, o, a, n, ne, no, na, r, rt, f, k, out_, s, stream)
# Hip's entry points allocate through torch: a stand-in with host memory behind it, as the stand-in runtime's hipMalloc
from _fake_torch import Tensor, install as fake_torch
if mode == "errors":
    T.check(lib.tray_init(0))
    nan = float("nan")
    mark("refused")
    for name, kw in [("w0", dict(w=0)), ("h0", dict(h=0)), ("r0", dict(r=0, rt=0)), ("r11", dict(r=11)), ("rt0", dict(rt=0)), ("rt_above_r", dict(r=3, rt=4)),
                     ("f4", dict(f=4)), ("k0", dict(k=0.0)), ("kneg", dict(k=-0.45)), ("knan", dict(k=nan)), ("n9", dict(n=9)),
                     ("null_even", dict(e=None)), ("null_odd", dict(o=None)), ("null_albedo", dict(a=None)), ("null_out", dict(out_=None)),
                     ("null_scratch", dict(s=None)), ("null_nb_even_array", dict(ne=None)), ("null_nb_odd_array", dict(no=None)),
                     ("null_nb_albedo_array", dict(na=None)), ("null_nb_film", dict(n=2, nbs=[nb[0], (nb[1][0], None, nb[1][2])])),
                     ("null_nb_albedo", dict(n=2, nbs=[nb[0], (nb[1][0], nb[1][1], None)])),
                     ("same_films", dict(o=even)), ("albedo_is_even", dict(a=even)), ("albedo_is_odd", dict(a=odd)), ("albedo_is_out", dict(a=out)),
                     ("albedo_is_scratch", dict(a=scratch)), ("centre_film_twice", dict(nbs=[(even, nb[0][1], nb[0][2])])),
                     ("centre_albedo_twice", dict(nbs=[(nb[0][0], nb[0][1], alb)])), ("nb_albedo_is_its_film", dict(nbs=[(nb[0][0], nb[0][1], nb[0][0])])),
                     ("nb_film_twice", dict(n=2, nbs=[nb[0], (nb[1][0], nb[0][0], nb[1][2])])),
                     ("nb_albedo_twice", dict(n=2, nbs=[nb[0], (nb[1][0], nb[1][1], nb[0][2])])),
                     ("out_is_even", dict(out_=even)), ("out_is_nb_film", dict(out_=nb[0][1])), ("out_is_nb_albedo", dict(out_=nb[0][2])),
                     ("scratch_is_nb_film", dict(s=nb[0][0])), ("scratch_is_nb_albedo", dict(s=nb[0][2])),
                     ("misaligned_even", dict(e=even + 4)), ("misaligned_albedo", dict(a=alb + 4)), ("misaligned_nb", dict(nbs=[(nb[0][0] + 8, nb[0][1], nb[0][2])])),
                     ("misaligned_nb_albedo", dict(nbs=[(nb[0][0], nb[0][1], nb[0][2] + 8)])), ("misaligned_out", dict(out_=out + 4)),
                     ("misaligned_scratch", dict(s=scratch + 12))]:
        rc = call(**kw)
        print("CASE", name, rc, "|", lib.tray_last_error().decode())
    mark("accepted")
    print("CASE smallest", call(w=1, h=1, n=0, ne=None, no=None, na=None, r=1, rt=1, f=0), "|")
elif mode == "launches":
    T.check(lib.tray_init(0))
    stream = C.c_void_p(0x5150)   # (the stand-in runtime only records the handle)
    mark("calls")
    for n in (0, 1, 3, 8):
        print("RC", n, call(n=n, stream=stream))
    print("RC_F1", call(w=33, h=17, n=2, r=3, rt=2, f=1, stream=stream))
    ne, no = arr([p[0] for p in nb[:2]]), arr([p[1] for p in nb[:2]])
    print("RC_T", lib.tray_denoise_temporal_device(W, H, even, odd, 2, ne, no, 7, 3, 3, 0.45, out, scratch, stream))
    C.CDLL(None).hipDeviceSynchronize()   # (a wait the log must show: the check below has teeth)
elif mode == "python":
    fake_torch()
    hip = T.Hip(0, seed=3)
    films = [np.ones((H, W, 4), np.float32) for _ in range(9)]
    pairs = [(films[0], films[1]), (films[2], films[3]), (films[4], films[5])]
    for kw in (dict(), dict(albedos=None), dict(albedos=films[6:9])):
        mark("denoise_temporal")
        o = hip.denoise_temporal(pairs, 1, **kw)
        print("OUT", type(o).__name__, o.shape, o.dtype)
    mark("one_frame")
    hip.denoise_temporal(pairs[:1], 0, albedos=films[6:7])
    mark("refused")
    for kw in (dict(albedos=films[6:8]), dict(albedos=[films[6], films[7], np.ones((H, W + 1, 4), np.float32)]), dict(albedos=[films[6], films[7], Tensor(films[8])])):
        try:
            hip.denoise_temporal(pairs, 1, **kw)
        except (ValueError, TypeError) as e:
            print("REFUSED", type(e).__name__, e)
else:
    fake_torch()
    d = %(tmp)r
    os.makedirs(os.path.join(d, "models"), exist_ok=True)
    open(os.path.join(d, "models", "cube.obj"), "w").write(scenes.cube_obj())
    s = scenes.cornell_box(64, 48, 16)
    s["film"].update({"frames": 4, "start_frame": 0, "end_frame": 3, "scene_time": 1.0})
    scene, rt, spp, fi = T.Scene.load_file(scenes.write_scene(s, os.path.join(d, "four_frames.json")))
    hip = T.Hip(0, seed=3)
    cfg = T.Config(d, "four_frames.json", spp, 1, fi, (0, 0))
    mark("one_range")
    hip.render_samples_device(scene, 0, (0, 0), 16, (0, 8), Tensor(np.zeros((48, 64, 4), np.float32)).data_ptr(), 0x5150)   # what one range launch looks like
    first_hit = hip.render_first_hit_device
    def spy(scene_, frame, select_blocks, spp_, rng, *a, **kw):
        print("ALBEDO", int(frame), tuple(int(v) for v in rng), int(spp_))
        return first_hit(scene_, frame, select_blocks, spp_, rng, *a, **kw)
    hip.render_first_hit_device = spy
    for kw in (dict(), dict(demodulate=True), dict(demodulate=True, feature_spp=4)):
        mark("sequence")
        Tensor.count = 0
        for frame, img in hip.render_sequence_denoised(scene, cfg, range(4), reach=1, **kw):
            print("FRAME", frame, img.shape, img.dtype)
        print("FILMS", Tensor.count)
    mark("refused")
    for kw in (dict(demodulate=True, feature_spp=0), dict(demodulate=True, feature_spp=32)):
        try:
            list(hip.render_sequence_denoised(scene, cfg, range(4), reach=1, **kw))
        except ValueError as e:
            print("REFUSED", e)
print("DONE")
'''


@pytest.fixture(scope="module")
def host_calls(tmp_path_factory, stub):
    """stub with fakehip_host_calls.c in front of the stand-in runtime"""
    lib = _stub._build(tmp_path_factory, "libfakehip_host_calls.so", "fakehip_host_calls.c", ["-ldl"])
    preload = ":".join(p for p in (lib, stub.args[0], os.environ.get("LD_PRELOAD", "")) if p)
    return lambda source, tmp_path, **env: stub(source, tmp_path, LD_PRELOAD=preload, **env)


def run(runner, tmp_path, mode):
    out, log = runner(DRIVER % {"root": ROOT, "tmp": str(tmp_path), "mode": mode}, tmp_path, FAKEHIP_DEVICES=1, FAKEHIP_TILE_KERNEL=None, TRAYHIP_MODE=None)
    assert "DONE" in out.stdout, out.stdout + out.stderr
    return out.stdout, log


def phases(log):
    """the log split at the driver's marks: [(mark name, lines)]; what precedes the first mark is dropped (tray_init, tray_scene_create)"""
    out = []
    for l in log:
        if l.startswith("mark"):
            out.append((l.split("=", 1)[1], []))
        elif out:
            out[-1][1].append(l)
    return out


PX = lambda w, h: (w * h + 255) // 256
TILES = lambda w, h: ((w + 31) // 32) * ((h + 15) // 16)
N_TILES = (64 // 8) * (48 // 8)


def tdm_call(w, h, n, f=3):
    """the launches of one demodulated call with n neighbours, streams cut off"""
    return [("tdm_prepare", -1, PX(w, h), 256), ("tdm_variance", 1, PX(w, h), 256), ("tdm_pass", f, TILES(w, h), 512)] * (n + 1)


def temporal_call(w, h, n):
    """... and of a tray_denoise_temporal_device call"""
    return [("prepare", 0, PX(w, h), 256), ("prepare", 1, PX(w, h), 256), ("pass", -1, TILES(w, h), 512)] * (n + 1)


def test_arguments_are_checked_before_any_device_call(host_calls, tmp_path):
    out, log = run(host_calls, tmp_path, "errors")
    cases = {}
    for l in out.splitlines():
        if l.startswith("CASE"):
            head, _, text = l.partition("|")
            cases[head.split()[1]] = (head.split()[2], text.strip())
    assert cases.pop("smallest")[0] == "0", out
    assert len(cases) == 42
    for name, (rc, text) in cases.items():
        assert rc == "-1", (name, rc)   # TRAY_E_INVALID
        assert text.startswith("tray_denoise_temporal_demodulated_device: ") and len(text) > 47, (name, text)
    (refused, lines), (_, ok_lines) = phases(log)
    assert refused == "refused" and lines == [], lines   # no launch, no wait, no copy, no fill
    # only the valid call launched anything: a 1 x 1 film without neighbours is one block of each kernel
    assert [e[:4] for e in launches(ok_lines)] == tdm_call(1, 1, 0, 0) and len(ok_lines) == 3, ok_lines


def test_scratch_bytes(stub, tmp_path):
    out, _ = run(stub, tmp_path, "launches")
    assert f"SCRATCH {70 * 40 * 128} 0 0 {65535 * 65535 * 128} {70 * 40 * 128}" in out, out   # the temporal call's; no 32-bit overflow


def test_a_call_is_three_launches_per_frame_in_order_and_nothing_between(host_calls, tmp_path):
    out, log = run(host_calls, tmp_path, "launches")
    for k in ("RC 0 0", "RC 1 0", "RC 3 0", "RC 8 0", "RC_F1 0", "RC_T 0"):
        assert k in out, out
    (_, lines), = phases(log)
    assert lines[-1] == "host call=hipDeviceSynchronize", lines[-3:]   # the driver's own wait after the last call
    lines = lines[:-1]
    ev = launches(lines)
    want = tdm_call(70, 40, 0) + tdm_call(70, 40, 1) + tdm_call(70, 40, 3) + tdm_call(70, 40, 8) + tdm_call(33, 17, 2, 1)
    assert len(want) == 3 * (1 + 2 + 4 + 9 + 3)
    # (every k_dn_prepare<1> among them is libtrayhip_tdemod.so's own: "tdm_variance" is read from a plain launch line)
    assert [e[:4] for e in ev[:len(want)]] == want, ev
    # tray_denoise_temporal_device launches what it launched before
    assert [e[:4] for e in ev[len(want):]] == temporal_call(70, 40, 2), ev[len(want):]
    assert all(e[4] == "0x5150" for e in ev), ev
    assert len(lines) == len(ev), [l for l in lines if l.startswith("host")]   # no wait, copy or fill, and nothing else


def test_denoise_temporal_defaults_launch_what_they_launched_before(stub, tmp_path):
    out, log = run(stub, tmp_path, "python")
    assert out.count("OUT ndarray (40, 70, 4) float32") == 3, out
    refused = [l for l in out.splitlines() if l.startswith("REFUSED")]
    assert [l.split()[1] for l in refused] == ["ValueError", "ValueError", "TypeError"] and all("denoise_temporal: " in l for l in refused), out
    ph = [(name, [e[:4] for e in launches(lines)], len(lines)) for name, lines in phases(log)]
    assert [n for n, _, _ in ph] == ["denoise_temporal"] * 3 + ["one_frame", "refused"]
    assert ph[0][1] == ph[1][1] == temporal_call(70, 40, 2) and ph[0][2] == ph[1][2] == 9   # as tests/test_temporal_stub.py has them on the parent commit
    assert ph[2][1] == tdm_call(70, 40, 2) and ph[2][2] == 9
    assert ph[3][1] == tdm_call(70, 40, 0)
    assert ph[4][1] == [] and ph[4][2] == 0


def test_a_sequence_renders_every_albedo_film_once_and_its_defaults_launch_what_they_launched_before(stub, tmp_path):
    out, log = run(stub, tmp_path, "sequence")
    blocks = out.split("FILMS")
    assert len(blocks) == 4
    for b in blocks[:3]:
        assert [l for l in b.splitlines() if l.startswith("FRAME")] == [f"FRAME {f} (48, 64, 4) float32" for f in range(4)], out
    albedo = lambda b: sorted(l for l in b.splitlines() if l.startswith("ALBEDO"))
    assert albedo(blocks[0]) == []
    assert albedo(blocks[1]) == [f"ALBEDO {f} (0, 16) 16" for f in range(4)]   # each frame's exactly once
    assert albedo(blocks[2]) == [f"ALBEDO {f} (0, 4) 16" for f in range(4)]
    # 2 reach + 1 pairs, rendered into again; with demodulate as many albedo films, and one shared normal / depth pair
    assert [b.split()[0] for b in blocks[1:]] == ["6", "11", "11"], out
    assert out.count("REFUSED render_sequence_denoised: feature_spp must lie in [1, 16]") == 2, out
    ph = phases(log)
    assert [n for n, _ in ph] == ["one_range"] + ["sequence"] * 3 + ["refused"]
    (one_range,), = [launches(ph[0][1])]
    assert one_range[0] == "other"
    render = [one_range] * 2   # a frame's two range launches
    ev = launches(ph[1][1])
    frame = lambda n: [e + ("0x5150",) for e in temporal_call(64, 48, n)]
    # the parent commit's log: tests/test_temporal_stub.py's expectation of the same sequence
    assert ev == render * 2 + frame(1) + render + frame(2) + render + frame(2) + frame(1), ev
    assert len(ph[1][1]) == len(ev)
    for _, lines in ph[2:4]:
        ev = launches(lines)
        feat = render + [("first_hit", -1, N_TILES, 256, "0x5150")]   # ... then the frame's one first-hit launch
        frame = lambda n: [e + ("0x5150",) for e in tdm_call(64, 48, n)]
        assert ev == feat * 2 + frame(1) + feat + frame(2) + feat + frame(2) + frame(1), ev
        assert sum(e[0] == "first_hit" for e in ev) == 4 and len(lines) == len(ev)
    assert ph[4][1] == []
