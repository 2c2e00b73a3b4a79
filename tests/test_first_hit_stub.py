"""tray_render_first_hit_device and tray_denoise_demodulated_device through the real library against the stand-in runtime (tests/stubs/fakehip.c),
as tests/test_guided_stub.py: every TRAY_E_INVALID / TRAY_E_UNSUPPORTED case of include/trayhip.h returns before any device call -- with
tests/stubs/fakehip_host_calls.c preloaded in front, which logs every wait, copy and fill --, the calls make 1 / 5 / 8 launches in stream order
with nothing between them, the scratch sizes, and Hip.denoise / Hip.render_denoised at their defaults launch what they launched before.
libtrayhip_firsthit.so's launches appear in the log as plain `launch` lines; the driver writes `mark` lines of its own between the phases. The
runs are made without FAKEHIP_TILE_KERNEL, which would read another kernel's arguments as the tile kernel's."""
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
def mark(name):
    with open(os.environ["FAKEHIP_LOG"], "a") as f:
        f.write("mark name=%%s\n" %% name)
W, H = 64, 48
FILM = W * H * 16
store = C.create_string_buffer(6 * (FILM + 16) + 16)
base = (C.addressof(store) + 15) & ~15
buf = lambda i: base + i * (FILM + 16)   # 16-byte aligned, pairwise different
even, odd, alb, out, nrm, dep = (buf(i) for i in range(6))
sizes = [int(lib.tray_denoise_demodulated_scratch_bytes(W, H, r2)) for r2 in (0, 5)]
print("SCRATCH", *sizes, *[int(lib.tray_denoise_demodulated_scratch_bytes(w, h, r2)) for r2 in (0, 1) for (w, h) in ((0, 7), (7, 0), (65535, 65535))])
scr = C.create_string_buffer(max(sizes) + 32)
scratch = (C.addressof(scr) + 15) & ~15
d = %(tmp)r
scenes.write_assets(d, cornell=(W, H, 16))
scene, rt, spp, fi = T.Scene.load_file(os.path.join(d, "cornell_box.json"))
def demod(w=W, h=H, e=even, o=odd, a=alb, r=7, f=3, k=0.45, r2=0, f2=1, k2=1.0, out_=out, s=scratch, stream=None):
    return lib.tray_denoise_demodulated_device(w, h, e, o, a, r, f, k, r2, f2, k2, out_, s, stream)
def first(dev, start=0, count=0, spp_=16, b=0, e=16, a=alb, n=nrm, z=dep, stream=None):
    return lib.tray_render_first_hit_device(dev, start, count, spp_, b, e, 3, a, n, z, stream)
nan, inf = float("nan"), float("inf")
if mode == "errors":
    T.check(lib.tray_init(0))
    dev = scene.device_scene(0, 0)
    mark("refused")
    for name, kw in [("null_scene", dict(dev=None)), ("null_albedo", dict(a=None)), ("null_normal", dict(n=None)), ("null_depth", dict(z=None)),
                     ("spp0", dict(spp_=0)), ("spp12", dict(spp_=12)), ("empty", dict(b=5, e=5)), ("reversed", dict(b=6, e=5)), ("past_spp", dict(e=17)),
                     ("same_an", dict(n=alb)), ("same_az", dict(z=alb)), ("same_nz", dict(z=nrm)), ("misaligned_albedo", dict(a=alb + 4)),
                     ("misaligned_normal", dict(n=nrm + 8)), ("misaligned_depth", dict(z=dep + 12))]:
        kw.setdefault("dev", dev)
        print("CASE", "first." + name, first(**kw), "|", lib.tray_last_error().decode())
    for kind, args in (("uniform", (1, 1, 1)), ("adaptive", (2, 4, 16))):
        T.check(lib.tray_scene_set_sampler(dev, *args))
        print("CASE", "first." + kind, first(dev), "|", lib.tray_last_error().decode())
    T.check(lib.tray_scene_set_sampler(dev, 0, 1, 1))
    for name, kw in [("w0", dict(w=0)), ("h0", dict(h=0)), ("r0", dict(r=0)), ("r11", dict(r=11)), ("f4", dict(f=4)), ("k0", dict(k=0.0)), ("kneg", dict(k=-1.0)),
                     ("knan", dict(k=nan)), ("kinf", dict(k=inf)), ("r2_11", dict(r2=11)), ("f2_4", dict(r2=5, f2=4)), ("k2_0", dict(r2=5, k2=0.0)),
                     ("k2_nan", dict(r2=5, k2=nan)), ("null_even", dict(e=None)), ("null_odd", dict(o=None)), ("null_albedo", dict(a=None)),
                     ("null_out", dict(out_=None)), ("null_scratch", dict(s=None)), ("same_films", dict(o=even)), ("albedo_is_even", dict(a=even)),
                     ("albedo_is_odd", dict(a=odd)), ("albedo_is_out", dict(a=out)), ("albedo_is_scratch", dict(a=scratch)), ("out_is_even", dict(out_=even)),
                     ("out_is_scratch", dict(out_=scratch)), ("misaligned_albedo", dict(a=alb + 4)), ("misaligned_even", dict(e=even + 8)),
                     ("misaligned_out", dict(out_=out + 4)), ("misaligned_scratch", dict(s=scratch + 12))]:
        print("CASE", "demod." + name, demod(**kw), "|", lib.tray_last_error().decode())
    mark("accepted")
    print("CASE ok_first", first(dev, b=5, e=13), "|")
    print("CASE ok_demod", demod(w=1, h=1, r=1, f=0), "|")
    print("CASE ok_demod2", demod(w=1, h=1, r=1, f=0, r2=1, f2=0), "|")
    print("CASE ok_f2_unread", demod(w=1, h=1, r=1, f=0, r2=0, f2=9, k2=nan), "|")   # (radius2 == 0: the second pass's arguments are not read)
elif mode == "launches":
    T.check(lib.tray_init(0))
    dev = scene.device_scene(0, 0)
    stream = C.c_void_p(0x5150)   # (the stand-in runtime only records the handle)
    mark("calls")
    print("RC_F", first(dev, b=0, e=8, stream=stream))
    print("RC_F2", first(dev, start=3, count=5, b=8, e=16, stream=stream))
    print("RC_D1", demod(stream=stream))
    print("RC_D2", demod(r2=5, stream=stream))
    print("RC_DN", lib.tray_denoise_device(W, H, even, odd, 7, 3, 0.45, out, scratch, stream))
    C.CDLL(None).hipDeviceSynchronize()   # (a wait the log must show: the check below has teeth)
else:
    # Hip.denoise and Hip.render_denoised allocate through torch: a stand-in with host memory behind it, as the stand-in runtime's hipMalloc
    from _fake_torch import Tensor, install as fake_torch
    fake_torch()
    cfg = T.Config(d, "cornell_box.json", spp, 1, fi, (0, 0))
    hip = T.Hip(0, seed=3)
    films = [np.ones((H, W, 4), np.float32) for _ in range(3)]
    for kw in (dict(), dict(albedo=films[2]), dict(albedo=films[2], passes=2)):
        mark("denoise")
        o = hip.denoise(films[0], films[1], **kw)
        print("OUT", type(o).__name__, o.shape, o.dtype)
    for kw in (dict(), dict(demodulate=True), dict(demodulate=True, feature_spp=4, passes=2)):
        mark("render")
        hip.render_denoised(scene, rt, cfg, **kw)
    mark("first_hit")
    f = hip.render_first_hit(scene, cfg, (2, 9))
    print("FILMS", sorted(f), [v.shape for v in f.values()])
    for kw in (dict(demodulate=True, error="filtered", threshold=0.1), dict(demodulate=True, feature_spp=0), dict(demodulate=True, feature_spp=32)):
        try:
            hip.render_denoised(scene, rt, cfg, **kw)
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
NIL = ("(nil)", "0", "0x0")
other = lambda grid: ("other", -1, grid, 256)
prepare = lambda w, h: [("prepare", 0, PX(w, h), 256), ("prepare", 1, PX(w, h), 256)]
one_pass = lambda w, h, f=3: prepare(w, h) + [("filter", f, TILES(w, h), 512)]
two_pass = lambda w, h, f=3, f2=1: prepare(w, h) + [("halves", f, TILES(w, h), 512)] + prepare(w, h) + [("guided", f2, TILES(w, h), 512)]
demod = lambda w, h, filt: [other(PX(w, h))] + filt + [other(PX(w, h))]   # k_fh_demodulate, the filter, k_fh_remodulate
N_TILES = (64 // 8) * (48 // 8)


def test_arguments_are_checked_before_any_device_call(host_calls, tmp_path):
    out, log = run(host_calls, tmp_path, "errors")
    cases = {}
    for l in out.splitlines():
        if l.startswith("CASE"):
            head, _, text = l.partition("|")
            cases[head.split()[1]] = (head.split()[2], text.strip())
    accepted = {k: cases.pop(k) for k in ("ok_first", "ok_demod", "ok_demod2", "ok_f2_unread")}
    assert len(cases) == 15 + 2 + 29
    for name, (rc, text) in cases.items():
        assert rc == ("-4" if name in ("first.uniform", "first.adaptive") else "-1"), (name, rc)   # TRAY_E_UNSUPPORTED, TRAY_E_INVALID
        assert len(text) > 16, (name, text)
        if name.startswith("demod."):
            assert text.startswith("tray_denoise_demodulated_device"), (name, text)
    assert all(rc == "0" for rc, _ in accepted.values()), accepted
    (refused, lines), (_, ok_lines) = phases(log)
    assert refused == "refused" and lines == [], lines   # no launch, no wait, no copy, no fill
    ev = launches(ok_lines)
    assert [e[:4] for e in ev] == [other(N_TILES)] + demod(1, 1, one_pass(1, 1, 0)) + demod(1, 1, two_pass(1, 1, 0, 0)) + demod(1, 1, one_pass(1, 1, 0)), ok_lines
    assert len(ok_lines) == len(ev), ok_lines


def test_scratch_bytes(stub, tmp_path):
    out, _ = run(stub, tmp_path, "launches")
    big = 65535 * 65535
    assert f"SCRATCH {64 * 48 * 80} {64 * 48 * 160} 0 0 {big * 80} 0 0 {big * 160}" in out, out   # the filter's 48 / 128 plus 32; no 32-bit overflow


def test_the_calls_make_1_5_and_8_launches_in_order_and_nothing_between(host_calls, tmp_path):
    out, log = run(host_calls, tmp_path, "launches")
    for k in ("RC_F 0", "RC_F2 0", "RC_D1 0", "RC_D2 0", "RC_DN 0"):
        assert k in out, out
    (_, lines), = phases(log)
    assert lines[-1] == "host call=hipDeviceSynchronize", lines[-3:]   # the driver's own wait after the last call
    lines = lines[:-1]
    ev = launches(lines)
    want = [other(N_TILES), other(5)] + demod(64, 48, one_pass(64, 48)) + demod(64, 48, two_pass(64, 48)) + one_pass(64, 48)
    assert [e[:4] for e in ev] == want, ev
    assert len(want) == 1 + 1 + 5 + 8 + 3
    assert all(e[4] == "0x5150" for e in ev), ev
    assert len(lines) == len(ev), [l for l in lines if l.startswith("host")]   # no wait, copy or fill, and nothing else


def test_python_defaults_launch_what_they_launched_before(stub, tmp_path):
    out, log = run(stub, tmp_path, "python")
    assert out.count("OUT ndarray (48, 64, 4) float32") == 3, out
    assert "FILMS ['albedo', 'depth', 'normal'] [(48, 64, 4), (48, 64, 4), (48, 64, 4)]" in out, out
    assert out.count("REFUSED render_denoised:") == 3, out
    ph = [(name, [e[:4] for e in launches(lines)]) for name, lines in phases(log)]
    assert [n for n, _ in ph] == ["denoise"] * 3 + ["render"] * 3 + ["first_hit"]
    assert ph[0][1] == one_pass(64, 48) and ph[1][1] == demod(64, 48, one_pass(64, 48)) and ph[2][1] == demod(64, 48, two_pass(64, 48))
    # render_denoised: a frame's two range launches, then the filter's -- with demodulate the first-hit launch and the two element-wise ones
    ranges = ph[3][1][:2]
    assert [e[0] for e in ranges] == ["other"] * 2 and ph[3][1] == ranges + one_pass(64, 48), ph[3]
    assert ph[4][1] == ranges + [other(N_TILES)] + demod(64, 48, one_pass(64, 48)), ph[4]
    assert ph[5][1] == ranges + [other(N_TILES)] + demod(64, 48, two_pass(64, 48)), ph[5]
    assert ph[6][1] == [other(N_TILES)], ph[6]   # (the refused calls launched nothing)
