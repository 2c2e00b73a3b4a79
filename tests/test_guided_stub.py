"""tray_denoise_guided_device and tray_denoise_two_pass_device through the real library against the stand-in runtime (tests/stubs/fakehip.c), as
tests/test_denoise_stub.py: every TRAY_E_INVALID case of include/trayhip.h with its tray_last_error text and nothing launched, the scratch
sizes, the five and six launches of the calls in their stated order on the caller's stream -- with tests/stubs/fakehip_host_calls.c preloaded in
front, which logs every wait, copy and fill, so that the log shows there is none between them --, and Hip.denoise / Hip.render_denoised at
their defaults launching what they launched before the second pass existed, with passes=2 the six launches. The runs are made without
FAKEHIP_TILE_KERNEL, which would read a filter's arguments as the tile kernel's."""
import os

import pytest

import _stub
from _stub import stub   # (a fixture)
from _guided_ref import launches

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
store = C.create_string_buffer(6 * (FILM + 16) + 16)
base = (C.addressof(store) + 15) & ~15
buf = lambda i: base + i * (FILM + 16)   # 16-byte aligned, pairwise different
even, odd, ga, gb, out = (buf(i) for i in range(5))
sizes = [int(fn(W, H)) for fn in (lib.tray_denoise_guided_scratch_bytes, lib.tray_denoise_two_pass_scratch_bytes)]
print("SCRATCH", *sizes, *[fn(*wh) for fn in (lib.tray_denoise_guided_scratch_bytes, lib.tray_denoise_two_pass_scratch_bytes)
                           for wh in ((0, 7), (7, 0), (65535, 65535))])
scr = C.create_string_buffer(max(sizes) + 32)
scratch = (C.addressof(scr) + 15) & ~15
def guided(w=W, h=H, e=even, o=odd, a=ga, b=gb, r=5, f=1, k=1.0, out_=out, s=scratch, stream=None):
    return lib.tray_denoise_guided_device(w, h, e, o, a, b, r, f, k, out_, s, stream)
def two(w=W, h=H, e=even, o=odd, r=7, f=3, k=0.45, r2=5, f2=1, k2=1.0, out_=out, s=scratch, stream=None):
    return lib.tray_denoise_two_pass_device(w, h, e, o, r, f, k, r2, f2, k2, out_, s, stream)
nan, inf = float("nan"), float("inf")
if mode == "errors":
    print("CASE init", lib.tray_init(0))
    shared = [("w0", dict(w=0)), ("h0", dict(h=0)), ("r0", dict(r=0)), ("r11", dict(r=11)), ("f4", dict(f=4)), ("k0", dict(k=0.0)), ("kneg", dict(k=-1.0)),
              ("knan", dict(k=nan)), ("kinf", dict(k=inf)), ("null_even", dict(e=None)), ("null_odd", dict(o=None)), ("null_out", dict(out_=None)),
              ("null_scratch", dict(s=None)), ("same_films", dict(o=even)), ("out_is_even", dict(out_=even)), ("out_is_odd", dict(out_=odd)),
              ("scratch_is_even", dict(s=even)), ("scratch_is_odd", dict(s=odd)), ("out_is_scratch", dict(out_=scratch)),
              ("misaligned_even", dict(e=even + 4)), ("misaligned_odd", dict(o=odd + 8)), ("misaligned_out", dict(out_=out + 4)),
              ("misaligned_scratch", dict(s=scratch + 12))]
    for name, kw in shared + [("null_guide_a", dict(a=None)), ("null_guide_b", dict(b=None)), ("same_guides", dict(b=ga)), ("out_is_guide_a", dict(out_=ga)),
                              ("out_is_guide_b", dict(out_=gb)), ("scratch_is_guide_a", dict(s=ga)), ("scratch_is_guide_b", dict(s=gb)),
                              ("misaligned_guide_a", dict(a=ga + 4)), ("misaligned_guide_b", dict(b=gb + 8))]:
        print("CASE", "guided." + name, guided(**kw), "|", lib.tray_last_error().decode())
    for name, kw in shared + [("r2_0", dict(r2=0)), ("r2_11", dict(r2=11)), ("f2_4", dict(f2=4)), ("k2_0", dict(k2=0.0)), ("k2_neg", dict(k2=-1.0)),
                              ("k2_nan", dict(k2=nan)), ("k2_inf", dict(k2=inf))]:
        print("CASE", "two." + name, two(**kw), "|", lib.tray_last_error().decode())
    print("LAUNCHED_NOTHING")
    print("CASE smallest_guided", guided(w=1, h=1, r=1, f=0), "|")
    print("CASE aliased_guide", guided(w=1, h=1, a=even, b=odd, r=1, f=0), "|")
    print("CASE smallest_two", two(w=1, h=1, r=1, f=0, r2=1, f2=0), "|")
elif mode == "launches":
    T.check(lib.tray_init(0))
    stream = C.c_void_p(0x5150)   # (the stand-in runtime only records the handle)
    print("RC_G", guided(stream=stream))
    print("RC_T", two(stream=stream))
    print("RC_T2", two(w=33, h=17, r=3, f=0, r2=10, f2=2))
    print("RC_DN", lib.tray_denoise_device(W, H, even, odd, 7, 3, 0.45, out, scratch, stream))
    C.CDLL(None).hipDeviceSynchronize()   # (a wait the log must show: the check below has teeth)
else:
    # Hip.denoise and Hip.render_denoised allocate through torch: a stand-in with host memory behind it, as the stand-in runtime's hipMalloc
    from _fake_torch import Tensor, install as fake_torch
    fake_torch()
    d = %(tmp)r
    scenes.write_assets(d, cornell=(64, 48, 16))
    scene, rt, spp, fi = T.Scene.load_file(os.path.join(d, "cornell_box.json"))
    cfg = T.Config(d, "cornell_box.json", spp, 1, fi, (0, 0))
    hip = T.Hip(0, seed=3)
    films = [np.ones((H, W, 4), np.float32) for _ in range(2)]
    for kw in (dict(), dict(passes=2), dict(passes=2, radius2=3, patch2=2, k2=0.7)):
        print("MARK denoise", sorted(kw))
        o = hip.denoise(*films, **kw)
        print("OUT", type(o).__name__, o.shape, o.dtype)
    print("MARK guided []")
    o = hip.denoise_guided(*films, *[f.copy() for f in films])
    print("OUT", type(o).__name__, o.shape, o.dtype)
    for kw in (dict(), dict(passes=2)):
        print("MARK render", sorted(kw))
        hip.render_denoised(scene, rt, cfg, **kw)
    for kw in (dict(passes=0), dict(passes=3)):
        try:
            hip.denoise(*films, **kw)
        except ValueError as e:
            print("REFUSED", e)
print("DONE")
'''


@pytest.fixture(scope="module")
def host_calls(tmp_path_factory, stub):
    """stub with fakehip_host_calls.c in front of the stand-in runtime"""
    lib = _stub._build(tmp_path_factory, "libfakehip_host_calls.so", "fakehip_host_calls.c", ["-ldl"])
    # (the keyword replaces what _stub.run put together, so whatever LD_PRELOAD the environment already holds is appended here as it is there)
    preload = ":".join(p for p in (lib, stub.args[0], os.environ.get("LD_PRELOAD", "")) if p)
    return lambda source, tmp_path, **env: stub(source, tmp_path, LD_PRELOAD=preload, **env)


def run(runner, tmp_path, mode):
    out, log = runner(DRIVER % {"root": ROOT, "tmp": str(tmp_path), "mode": mode}, tmp_path, FAKEHIP_DEVICES=1, FAKEHIP_TILE_KERNEL=None, TRAYHIP_MODE=None)
    assert "DONE" in out.stdout, out.stdout + out.stderr
    return out.stdout, log


PX = lambda w, h: (w * h + 255) // 256
TILES = lambda w, h: ((w + 31) // 32) * ((h + 15) // 16)
NIL = ("(nil)", "0", "0x0")
prepare = lambda w, h: [("prepare", 0, PX(w, h), 256), ("prepare", 1, PX(w, h), 256)]
one_pass = lambda w, h, f=3: prepare(w, h) + [("filter", f, TILES(w, h), 512)]
guided = lambda w, h, f=1: prepare(w, h) * 2 + [("guided", f, TILES(w, h), 512)]
two_pass = lambda w, h, f=3, f2=1: prepare(w, h) + [("halves", f, TILES(w, h), 512)] + prepare(w, h) + [("guided", f2, TILES(w, h), 512)]


def test_arguments_are_checked_before_any_device_call(host_calls, tmp_path):
    out, log = run(host_calls, tmp_path, "errors")
    refused, accepted = out.split("LAUNCHED_NOTHING")
    cases = {}
    for l in refused.splitlines():
        if l.startswith("CASE"):
            head, _, text = l.partition("|")
            cases[head.split()[1]] = (head.split()[2], text.strip())
    assert cases.pop("init")[0] == "0"
    assert len(cases) == (23 + 9) + (23 + 7)
    for name, (rc, text) in cases.items():
        assert rc == "-1", (name, rc)   # TRAY_E_INVALID
        who = "tray_denoise_guided_device" if name.startswith("guided.") else "tray_denoise_two_pass_device"
        assert text.startswith(who) and len(text) > len(who) + 8, (name, text)
    assert [l.split()[1:3] for l in accepted.splitlines() if l.startswith("CASE")] == [["smallest_guided", "0"], ["aliased_guide", "0"], ["smallest_two", "0"]]
    # only the valid calls launched anything or touched the device in any other way: 1 x 1 films are one block of each kernel
    ev = launches(log)
    assert [e[:4] for e in ev] == guided(1, 1, 0) * 2 + two_pass(1, 1, 0, 0), log
    assert not any(l.startswith("host") for l in log), log


def test_scratch_bytes(stub, tmp_path):
    out, _ = run(stub, tmp_path, "launches")
    big = 65535 * 65535
    assert f"SCRATCH {70 * 40 * 96} {70 * 40 * 128} 0 0 {big * 96} 0 0 {big * 128}" in out, out   # (no 32-bit overflow)


def test_the_calls_make_their_launches_in_order_on_the_callers_stream_and_nothing_between(host_calls, tmp_path):
    out, log = run(host_calls, tmp_path, "launches")
    for k in ("RC_G 0", "RC_T 0", "RC_T2 0", "RC_DN 0"):
        assert k in out, out
    first = next(i for i, l in enumerate(log) if l.startswith(("denoise", "guide")))
    assert not any(l.startswith(("denoise", "guide", "launch")) for l in log[:first])
    assert log[-1] == "host call=hipDeviceSynchronize", log[-3:]   # the driver's own wait after the last call
    log = log[first:-1]   # (tray_init is over)
    # ("guided" / "halves" lines exist because the stand-in runtime's test for libtrayhip_guide's file name also matches libtrayhip_guided.so: if
    # that test ever changes, k_gdn_filter's launches become plain "launch" lines, "other" here, and this comparison says so)
    ev = launches(log)
    want = guided(70, 40) + two_pass(70, 40)
    assert [e[:4] for e in ev[:11]] == want and all(e[4] == "0x5150" for e in ev[:11]), ev
    assert [e[:4] for e in ev[11:17]] == two_pass(33, 17, 0, 2) and all(e[4] in NIL for e in ev[11:17]), ev
    # tray_denoise_device on the same films: its three lines, as before
    assert [e[:4] for e in ev[17:]] == one_pass(70, 40) and all(e[4] == "0x5150" for e in ev[17:]), ev
    assert len(log) == len(ev), [l for l in log if l.startswith("host")]   # no wait, copy or fill, and nothing else


def test_python_defaults_launch_what_they_launched_before(stub, tmp_path):
    out, log = run(stub, tmp_path, "python")
    assert out.count("OUT ndarray (40, 70, 4) float32") == 4, out
    assert out.count("REFUSED denoise: passes must be 1 or 2") == 2, out
    ev = launches(log)
    assert all(e[4] == "0x5150" for e in ev)
    ev = [e[:4] for e in ev]
    want = one_pass(70, 40) + two_pass(70, 40) + two_pass(70, 40, 3, 2) + guided(70, 40)
    assert ev[:len(want)] == want, ev
    rest = ev[len(want):]
    # render_denoised: a frame's two range launches, then the filter's
    assert [e[0] for e in rest[:2]] == ["other"] * 2 and rest[2:5] == one_pass(64, 48), rest
    assert [e[0] for e in rest[5:7]] == ["other"] * 2 and rest[5:7] == rest[:2] and rest[7:] == two_pass(64, 48), rest
