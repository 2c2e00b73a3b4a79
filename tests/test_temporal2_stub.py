"""tray_denoise_temporal_halves_device, tray_denoise_temporal_guided_device, tray_denoise_temporal_two_pass_device, Hip.denoise_temporal(passes=2)
and Hip.render_sequence_denoised(passes=2) through the real library against the stand-in runtime (tests/stubs/fakehip.c), as
tests/test_tdemod_stub.py: every TRAY_E_INVALID case of include/trayhip.h returns before any device call -- with tests/stubs/fakehip_host_calls.c
preloaded in front, which logs every wait, copy and fill --, the scratch sizes, each call's launches for N = 0, 1, 2, 8 in the header's order with
nothing between them -- the kernels of libtrayhip_t2pass.so are plain `launch` lines, told apart by kernel symbol --, the defaults of the Python
entry points launching what they launched before, and a two-pass sequence computing every frame's own first-pass halves exactly once. The runs are
made without FAKEHIP_TILE_KERNEL, which would read another kernel's arguments as the tile kernel's."""
import os

import pytest

import _stub
from _stub import stub   # (a fixture)
from _temporal2_ref import launches

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
store = C.create_string_buffer(48 * (FILM + 16) + 16)
base = (C.addressof(store) + 15) & ~15
buf = lambda i: base + i * (FILM + 16)   # 16-byte aligned, pairwise different
even, odd, ga, gb, out, fa, fb = (buf(i) for i in range(7))
nb = [tuple(buf(7 + 4 * j + i) for i in range(4)) for j in range(9)]   # a neighbour's even, odd, guide_a, guide_b
sizes = [getattr(lib, "tray_denoise_temporal_%%s_scratch_bytes" %% n) for n in ("halves", "guided", "two_pass")]
print("SCRATCH", *[int(s(W, H)) for s in sizes], *[int(s(0, 7)) + int(s(7, 0)) for s in sizes], *[int(s(65535, 65535)) for s in sizes],
      int(lib.tray_denoise_temporal_scratch_bytes(W, H)))
scr = C.create_string_buffer(max(int(s(W, H)) for s in sizes) + 32)
scratch = (C.addressof(scr) + 15) & ~15
arr = lambda ptrs: (C.c_void_p * max(len(ptrs), 1))(*ptrs)
ZERO = object()   # "build the host array from nbs"
def arrays(nbs, given):
    return [arr([p[i] for p in nbs]) if g is ZERO else g for i, g in enumerate(given)]
def halves(w=W, h=H, e=even, o=odd, n=1, nbs=None, ne=ZERO, no=ZERO, r=7, rt=3, f=3, k=0.45, a=fa, b=fb, s=scratch, stream=None):
    ne, no = arrays(nb[:n] if nbs is None else nbs, (ne, no))
    return lib.tray_denoise_temporal_halves_device(w, h, e, o, n, ne, no, r, rt, f, k, a, b, s, stream)
def guided(w=W, h=H, e=even, o=odd, ga_=ga, gb_=gb, n=1, nbs=None, ne=ZERO, no=ZERO, na=ZERO, nb_=ZERO, r=5, rt=3, f=1, k=1.0, out_=out, s=scratch,
           stream=None):
    ne, no, na, nb_ = arrays(nb[:n] if nbs is None else nbs, (ne, no, na, nb_))
    return lib.tray_denoise_temporal_guided_device(w, h, e, o, ga_, gb_, n, ne, no, na, nb_, r, rt, f, k, out_, s, stream)
def two_pass(w=W, h=H, e=even, o=odd, n=1, nbs=None, ne=ZERO, no=ZERO, r=7, rt=3, f=3, k=0.45, r2=5, rt2=3, f2=1, k2=1.0, out_=out, s=scratch, stream=None):
    ne, no = arrays(nb[:n] if nbs is None else nbs, (ne, no))
    return lib.tray_denoise_temporal_two_pass_device(w, h, e, o, n, ne, no, r, rt, f, k, r2, rt2, f2, k2, out_, s, stream)
# Hip's entry points allocate through torch: a stand-in with host memory behind it, as the stand-in runtime's hipMalloc
from _fake_torch import Tensor, install as fake_torch
if mode == "errors":
    T.check(lib.tray_init(0))
    nan, inf = float("nan"), float("inf")
    first = [("w0", dict(w=0)), ("h0", dict(h=0)), ("r0", dict(r=0, rt=0)), ("r11", dict(r=11)), ("rt0", dict(rt=0)), ("rt_above_r", dict(r=2, rt=3)),
             ("f4", dict(f=4)), ("k0", dict(k=0.0)), ("kneg", dict(k=-0.45)), ("knan", dict(k=nan)), ("kinf", dict(k=inf)), ("n9", dict(n=9)),
             ("null_even", dict(e=None)), ("null_odd", dict(o=None)), ("null_scratch", dict(s=None)), ("null_nb_even_array", dict(ne=None)),
             ("null_nb_odd_array", dict(no=None)), ("null_nb_film", dict(n=2, nbs=[nb[0], (nb[1][0], None, nb[1][2], nb[1][3])])),
             ("same_films", dict(o=even)), ("nb_same_films", dict(nbs=[(nb[0][0], nb[0][0], nb[0][2], nb[0][3])])),
             ("scratch_is_even", dict(s=even)), ("scratch_is_nb_film", dict(s=nb[0][1])),
             ("misaligned_even", dict(e=even + 4)), ("misaligned_nb", dict(nbs=[(nb[0][0] + 8, nb[0][1], nb[0][2], nb[0][3])])),
             ("misaligned_scratch", dict(s=scratch + 12))]
    one_out = [("null_out", dict(out_=None)), ("out_is_even", dict(out_=even)), ("out_is_nb_film", dict(out_=nb[0][1])), ("out_is_scratch", dict(out_=scratch)),
               ("misaligned_out", dict(out_=out + 4))]
    cases = {
        "halves": (halves, first + [("centre_film_twice", dict(nbs=[(even, nb[0][1], 0, 0)])), ("null_fa", dict(a=None)), ("null_fb", dict(b=None)),
                                    ("fa_is_fb", dict(b=fa)), ("fa_is_even", dict(a=even)), ("fb_is_nb_film", dict(b=nb[0][0])), ("fa_is_scratch", dict(a=scratch)),
                                    ("misaligned_fa", dict(a=fa + 4)), ("misaligned_fb", dict(b=fb + 8))]),
        "guided": (guided, first + one_out + [("null_guide_a", dict(ga_=None)), ("null_guide_b", dict(gb_=None)), ("null_nb_guide_a_array", dict(na=None)),
                                              ("null_nb_guide_b_array", dict(nb_=None)), ("null_nb_guide", dict(nbs=[(nb[0][0], nb[0][1], nb[0][2], None)])),
                                              ("same_guides", dict(gb_=ga)), ("nb_same_guides", dict(nbs=[(nb[0][0], nb[0][1], nb[0][2], nb[0][2])])),
                                              ("out_is_guide", dict(out_=gb)), ("out_is_nb_guide", dict(out_=nb[0][3])), ("scratch_is_guide", dict(s=ga)),
                                              ("scratch_is_nb_guide", dict(s=nb[0][2])), ("misaligned_guide", dict(ga_=ga + 4)),
                                              ("misaligned_nb_guide", dict(nbs=[(nb[0][0], nb[0][1], nb[0][2], nb[0][3] + 8)]))]),
        "two_pass": (two_pass, first + one_out + [("centre_film_twice", dict(nbs=[(even, nb[0][1], 0, 0)])), ("r2_0", dict(r2=0, rt2=0)), ("r2_11", dict(r2=11)),
                                                  ("rt2_0", dict(rt2=0)), ("rt2_above_r2", dict(r2=3, rt2=4)), ("f2_4", dict(f2=4)), ("k2_0", dict(k2=0.0)),
                                                  ("k2_neg", dict(k2=-1.0)), ("k2_nan", dict(k2=nan)), ("k2_inf", dict(k2=inf))]),
    }
    mark("refused")
    for call_name, (fn, cs) in cases.items():
        for name, kw in cs:
            rc = fn(**kw)
            print("CASE", call_name, name, rc, "|", lib.tray_last_error().decode())
    small = dict(w=1, h=1, n=0, ne=None, no=None, r=1, rt=1, f=0)
    for call_name, fn, kw in (("halves", halves, small), ("guided", guided, dict(small, na=None, nb_=None)), ("two_pass", two_pass, dict(small, r2=1, rt2=1, f2=0)),
                              ("guided_own", guided, dict(ga_=even, gb_=odd, nbs=[(nb[0][0], nb[0][1], nb[0][0], nb[0][1])]))):
        mark("accepted_" + call_name)
        print("OK", call_name, fn(**kw), "|")
elif mode == "launches":
    T.check(lib.tray_init(0))
    stream = C.c_void_p(0x5150)   # (the stand-in runtime only records the handle)
    for call_name, fn in (("halves", halves), ("guided", guided), ("two_pass", two_pass)):
        for n in (0, 1, 2, 8):
            mark("%%s_%%d" %% (call_name, n))
            print("RC", call_name, n, fn(n=n, stream=stream))
    mark("other_patches")
    print("RC_F", halves(w=33, h=17, n=2, r=3, rt=2, f=1, stream=stream), guided(w=33, h=17, n=2, r=3, rt=2, f=0, stream=stream),
          two_pass(w=33, h=17, n=2, r=3, rt=2, f=2, r2=3, rt2=2, f2=0, stream=stream))
    C.CDLL(None).hipDeviceSynchronize()   # (a wait the log must show: the check below has teeth)
elif mode == "python":
    fake_torch()
    hip = T.Hip(0, seed=3)
    films = [np.ones((H, W, 4), np.float32) for _ in range(12)]
    pairs = [(films[0], films[1]), (films[2], films[3]), (films[4], films[5])]
    guides = [(films[6], films[7]), (films[8], films[9]), (films[10], films[11])]
    for kw in (dict(), dict(passes=1), dict(passes=2), dict(passes=2, radius2=3, radius_t2=2, patch2=0, k2=0.5)):
        mark("denoise_temporal")
        o = hip.denoise_temporal(pairs, 1, **kw)
        print("OUT", type(o).__name__, o.shape, o.dtype)
    mark("one_frame")
    hip.denoise_temporal(pairs[:1], 0, passes=2)
    mark("denoise_two_pass")
    hip.denoise(films[0], films[1], passes=2)
    mark("halves")
    o = hip.denoise_temporal_halves(pairs, 1)
    print("HALVES", type(o).__name__, len(o), type(o[0]).__name__, o[0].shape, o[1].dtype)
    mark("guided")
    o = hip.denoise_temporal_guided(pairs, guides, 1)
    print("OUT", type(o).__name__, o.shape, o.dtype)
    mark("tensors")
    t = lambda prs: [(Tensor(a), Tensor(b)) for a, b in prs]
    print("TENSORS", type(hip.denoise_temporal(t(pairs), 1, passes=2)).__name__, type(hip.denoise_temporal_halves(t(pairs), 1)[1]).__name__,
          type(hip.denoise_temporal_guided(t(pairs), t(guides), 1)).__name__)
    mark("refused")
    for fn in (lambda: hip.denoise_temporal(pairs, 1, passes=2, albedos=films[6:9]), lambda: hip.denoise_temporal(pairs, 1, passes=3),
               lambda: hip.denoise_temporal_guided(pairs, guides[:2], 1), lambda: hip.denoise_temporal_guided(pairs, t(guides), 1),
               lambda: hip.denoise_temporal_halves(pairs, 3)):
        try:
            fn()
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
    for kw in (dict(), dict(passes=2), dict(passes=2, radius2=3, radius_t2=2, patch2=0)):
        mark("sequence")
        Tensor.count = 0
        for frame, img in hip.render_sequence_denoised(scene, cfg, range(4), reach=1, **kw):
            print("FRAME", frame, img.shape, img.dtype)
        print("FILMS", Tensor.count)
    mark("refused")
    try:
        list(hip.render_sequence_denoised(scene, cfg, range(4), reach=1, passes=2, demodulate=True))
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


def prepare(w, h):
    """tray_denoise_device's two preparing launches, streams cut off"""
    return [("prepare", 0, PX(w, h), 256), ("prepare", 1, PX(w, h), 256)]


def halves_call(w, h, n, f=3):
    """the 3 (N + 1) launches of tray_denoise_temporal_halves_device as include/trayhip.h orders them"""
    return (prepare(w, h) + [("t2p_halves", f, TILES(w, h), 512)]) * (n + 1)


def guided_call(w, h, n, f=1):
    """the 5 (N + 1) launches of tray_denoise_temporal_guided_device: the values' preparing ones, the guide's, the pass"""
    return (prepare(w, h) * 2 + [("t2p_guided", f, TILES(w, h), 512)]) * (n + 1)


def single_halves(w, h, f=3):
    """tray_denoise_halves_device over every block: a neighbour's own pilot"""
    return prepare(w, h) + [("halves", f, TILES(w, h), 512)]


def two_pass_call(w, h, n, f=3, f2=1):
    """the 9 N + 6 launches of tray_denoise_temporal_two_pass_device"""
    guided = [("t2p_guided", f2, TILES(w, h), 512)]
    return halves_call(w, h, n, f) + prepare(w, h) + guided + (single_halves(w, h, f) + prepare(w, h) + guided) * n


def temporal_call(w, h, n):
    """... and of a tray_denoise_temporal_device call, as tests/test_temporal_stub.py has them"""
    return [("prepare", 0, PX(w, h), 256), ("prepare", 1, PX(w, h), 256), ("pass", -1, TILES(w, h), 512)] * (n + 1)


CALLS = {"halves": halves_call, "guided": guided_call, "two_pass": two_pass_call}
PREFIX = {"halves": "tray_denoise_temporal_halves_device", "guided": "tray_denoise_temporal_guided_device", "two_pass": "tray_denoise_temporal_two_pass_device"}


def test_arguments_are_checked_before_any_device_call(host_calls, tmp_path):
    out, log = run(host_calls, tmp_path, "errors")
    cases = [l for l in out.splitlines() if l.startswith("CASE")]
    assert [sum(l.split()[1] == c for l in cases) for c in ("halves", "guided", "two_pass")] == [34, 43, 40], out
    for l in cases:
        head, _, text = l.partition("|")
        _, call, name, rc = head.split()
        assert rc == "-1", (call, name, rc)   # TRAY_E_INVALID
        assert text.strip().startswith(PREFIX[call]) and len(text.strip()) > len(PREFIX[call]) + 10, (call, name, text)
    assert [l.split()[2] for l in out.splitlines() if l.startswith("OK")] == ["0"] * 4, out
    ph = phases(log)
    assert [n for n, _ in ph] == ["refused", "accepted_halves", "accepted_guided", "accepted_two_pass", "accepted_guided_own"]
    assert ph[0][1] == [], ph[0][1]   # no launch, no wait, no copy, no fill
    # only the valid calls launched anything: a 1 x 1 film without neighbours is one block of each kernel
    for (name, lines), want in zip(ph[1:], (halves_call(1, 1, 0, 0), guided_call(1, 1, 0, 0), two_pass_call(1, 1, 0, 0, 0), guided_call(70, 40, 1))):
        assert [e[:4] for e in launches(lines)] == want and len(lines) == len(want), (name, lines)


def test_scratch_bytes(stub, tmp_path):
    out, _ = run(stub, tmp_path, "launches")
    px, big = 70 * 40, 65535 * 65535
    # fixed per pixel whatever N is; the halves call's is the temporal call's; no 32-bit overflow
    assert f"SCRATCH {px * 128} {px * 176} {px * 256} 0 0 0 {big * 128} {big * 176} {big * 256} {px * 128}" in out, out


def test_each_call_launches_what_the_header_states_in_order_and_nothing_between(host_calls, tmp_path):
    out, log = run(host_calls, tmp_path, "launches")
    assert out.count("RC ") == 12 and all(l.split()[3] == "0" for l in out.splitlines() if l.startswith("RC ")) and "RC_F 0 0 0" in out, out
    ph = phases(log)
    assert [n for n, _ in ph] == [f"{c}_{n}" for c in CALLS for n in (0, 1, 2, 8)] + ["other_patches"]
    count = {"halves": lambda n: 3 * (n + 1), "guided": lambda n: 5 * (n + 1), "two_pass": lambda n: 9 * n + 6}
    for (name, lines), (c, n) in zip(ph, [(c, n) for c in CALLS for n in (0, 1, 2, 8)]):
        ev = launches(lines)
        assert [e[:4] for e in ev] == CALLS[c](70, 40, n), (name, ev)
        assert len(lines) == len(ev) == count[c](n), (name, [l for l in lines if l.startswith("host")])   # no wait, copy or fill, and nothing else
        assert all(e[4] == "0x5150" for e in ev), (name, ev)
    lines = ph[-1][1]
    assert lines[-1] == "host call=hipDeviceSynchronize", lines[-3:]   # the driver's own wait after the last call
    ev = launches(lines[:-1])
    assert [e[:4] for e in ev] == halves_call(33, 17, 2, 1) + guided_call(33, 17, 2, 0) + two_pass_call(33, 17, 2, 2, 0), ev
    assert len(lines) - 1 == len(ev)


def test_python_entry_points_and_their_defaults(stub, tmp_path):
    out, log = run(stub, tmp_path, "python")
    assert out.count("OUT ndarray (40, 70, 4) float32") == 5, out
    assert "HALVES tuple 2 ndarray (40, 70, 4) float32" in out and "TENSORS Tensor Tensor Tensor" in out, out
    refused = [l for l in out.splitlines() if l.startswith("REFUSED")]
    assert [l.split()[1] for l in refused] == ["ValueError", "ValueError", "ValueError", "TypeError", "ValueError"], out
    assert "denoise_temporal: passes=2" in refused[0] and "passes must be 1 or 2" in refused[1], out
    ph = [(name, [e[:4] for e in launches(lines)], len(lines)) for name, lines in phases(log)]
    assert [n for n, _, _ in ph] == ["denoise_temporal"] * 4 + ["one_frame", "denoise_two_pass", "halves", "guided", "tensors", "refused"]
    # the defaults launch what they launched before: tests/test_temporal_stub.py's and tests/test_guided_stub.py's expectations
    assert ph[0][1] == ph[1][1] == temporal_call(70, 40, 2) and ph[0][2] == ph[1][2] == 9
    assert ph[2][1] == two_pass_call(70, 40, 2) and ph[2][2] == 24
    assert ph[3][1] == two_pass_call(70, 40, 2, 3, 0)
    assert ph[4][1] == two_pass_call(70, 40, 0)
    assert ph[5][1] == prepare(70, 40) + [("halves", 3, TILES(70, 40), 512)] + prepare(70, 40) + [("guided", 1, TILES(70, 40), 512)] and ph[5][2] == 6
    assert ph[6][1] == halves_call(70, 40, 2)
    assert ph[7][1] == guided_call(70, 40, 2)
    assert ph[8][1] == two_pass_call(70, 40, 2) + halves_call(70, 40, 2) + guided_call(70, 40, 2)
    assert ph[9][1] == [] and ph[9][2] == 0


def test_a_two_pass_sequence_computes_every_frames_own_halves_once_and_the_defaults_launch_what_they_did(stub, tmp_path):
    out, log = run(stub, tmp_path, "sequence")
    blocks = out.split("FILMS")
    assert len(blocks) == 4
    for b in blocks[:3]:
        assert [l for l in b.splitlines() if l.startswith("FRAME")] == [f"FRAME {f} (48, 64, 4) float32" for f in range(4)], out
    # 2 reach + 1 pairs, rendered into again; with passes=2 as many pairs of halves, and one pair for the centre's halves over all frames
    assert [b.split()[0] for b in blocks[1:]] == ["6", "14", "14"], out
    assert out.count("REFUSED render_sequence_denoised: passes=2") == 1, out
    ph = phases(log)
    assert [n for n, _ in ph] == ["one_range"] + ["sequence"] * 3 + ["refused"]
    (one_range,), = [launches(ph[0][1])]
    assert one_range[0] == "other"
    render = [one_range] * 2   # a frame's two range launches
    on_stream = lambda events: [e + ("0x5150",) for e in events]
    ev = launches(ph[1][1])
    frame = lambda n: on_stream(temporal_call(64, 48, n))
    # the parent commit's log: tests/test_temporal_stub.py's expectation of the same sequence
    assert ev == render * 2 + frame(1) + render + frame(2) + render + frame(2) + frame(1), ev
    assert len(ph[1][1]) == len(ev)
    for (_, lines), f2 in zip(ph[2:4], (1, 0)):
        ev = launches(lines)
        own = render + on_stream(single_halves(64, 48))   # a frame is rendered, then its own halves are filtered: once
        frame = lambda n: on_stream(halves_call(64, 48, n) + guided_call(64, 48, n, f2))
        assert ev == own * 2 + frame(1) + own + frame(2) + own + frame(2) + frame(1), ev
        assert sum(e[0] == "halves" for e in ev) == 4 and len(lines) == len(ev)
    assert ph[4][1] == []
