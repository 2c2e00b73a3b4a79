"""tray_denoise_temporal_demodulated_halves_device, _guided_device and _two_pass_device, Hip.denoise_temporal_demodulated, its halves and guided
forms and Hip.render_sequence_demodulated through the real library against the stand-in runtime (tests/stubs/fakehip.c), as
tests/test_temporal2_stub.py: every TRAY_E_INVALID case of include/trayhip.h returns before any device call -- with
tests/stubs/fakehip_host_calls.c preloaded in front, which logs every wait, copy and fill --, the scratch sizes, each call's launches for
N = 0, 1, 2, 8 in the two-pass temporal call's order and count with nothing between them -- the kernels of libtrayhip_td2pass.so and
libtrayhip_t2pass.so are plain `launch` lines, told apart by kernel symbol; the library's name is logged under no other library's prefix --,
the Python entry points' launches, a four-frame sequence computing every frame's own halves and albedo film exactly once, and the defaults of
the existing entry points launching what the existing stub files expect. The runs are made without FAKEHIP_TILE_KERNEL, which would read
another kernel's arguments as the tile kernel's."""
import os

import pytest

import _stub
from _stub import stub   # (a fixture)
from _td2pass_ref import launches

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
store = C.create_string_buffer(56 * (FILM + 16) + 16)
base = (C.addressof(store) + 15) & ~15
buf = lambda i: base + i * (FILM + 16)   # 16-byte aligned, pairwise different
even, odd, alb, ga, gb, out, fa, fb = (buf(i) for i in range(8))
nb = [tuple(buf(8 + 5 * j + i) for i in range(5)) for j in range(9)]   # a neighbour's even, odd, albedo, guide_a, guide_b
sizes = [getattr(lib, "tray_denoise_temporal_demodulated_%%s_scratch_bytes" %% n) for n in ("halves", "guided", "two_pass")]
print("SCRATCH", *[int(s(W, H)) for s in sizes], *[int(s(0, 7)) + int(s(7, 0)) for s in sizes], *[int(s(65535, 65535)) for s in sizes])
scr = C.create_string_buffer(max(int(s(W, H)) for s in sizes) + 32)
scratch = (C.addressof(scr) + 15) & ~15
arr = lambda ptrs: (C.c_void_p * max(len(ptrs), 1))(*ptrs)
ZERO = object()   # "build the host array from nbs"
def arrays(nbs, given):
    return [arr([p[i] for p in nbs]) if g is ZERO else g for i, g in enumerate(given)]
def halves(w=W, h=H, e=even, o=odd, al=alb, n=1, nbs=None, ne=ZERO, no=ZERO, nal=ZERO, r=7, rt=3, f=3, k=0.45, a=fa, b=fb, s=scratch, stream=None):
    ne, no, nal = arrays(nb[:n] if nbs is None else nbs, (ne, no, nal))
    return lib.tray_denoise_temporal_demodulated_halves_device(w, h, e, o, al, n, ne, no, nal, r, rt, f, k, a, b, s, stream)
def guided(w=W, h=H, e=even, o=odd, al=alb, ga_=ga, gb_=gb, n=1, nbs=None, ne=ZERO, no=ZERO, nal=ZERO, na=ZERO, nb_=ZERO, r=5, rt=3, f=1, k=1.0, out_=out,
           s=scratch, stream=None):
    ne, no, nal, na, nb_ = arrays(nb[:n] if nbs is None else nbs, (ne, no, nal, na, nb_))
    return lib.tray_denoise_temporal_demodulated_guided_device(w, h, e, o, al, ga_, gb_, n, ne, no, nal, na, nb_, r, rt, f, k, out_, s, stream)
def two_pass(w=W, h=H, e=even, o=odd, al=alb, n=1, nbs=None, ne=ZERO, no=ZERO, nal=ZERO, r=7, rt=3, f=3, k=0.45, r2=5, rt2=3, f2=1, k2=1.0, out_=out,
             s=scratch, stream=None):
    ne, no, nal = arrays(nb[:n] if nbs is None else nbs, (ne, no, nal))
    return lib.tray_denoise_temporal_demodulated_two_pass_device(w, h, e, o, al, n, ne, no, nal, r, rt, f, k, r2, rt2, f2, k2, out_, s, stream)
# Hip's entry points allocate through torch: a stand-in with host memory behind it, as the stand-in runtime's hipMalloc
from _fake_torch import Tensor, install as fake_torch
def with_film(j, i, p):
    t = list(nb[j]); t[i] = p; return tuple(t)
if mode == "errors":
    T.check(lib.tray_init(0))
    nan, inf = float("nan"), float("inf")
    first = [("w0", dict(w=0)), ("h0", dict(h=0)), ("r0", dict(r=0, rt=0)), ("r11", dict(r=11)), ("rt0", dict(rt=0)), ("rt_above_r", dict(r=2, rt=3)),
             ("f4", dict(f=4)), ("k0", dict(k=0.0)), ("kneg", dict(k=-0.45)), ("knan", dict(k=nan)), ("kinf", dict(k=inf)), ("n9", dict(n=9)),
             ("null_even", dict(e=None)), ("null_odd", dict(o=None)), ("null_albedo", dict(al=None)), ("null_scratch", dict(s=None)),
             ("null_nb_even_array", dict(ne=None)), ("null_nb_odd_array", dict(no=None)), ("null_nb_albedo_array", dict(nal=None)),
             ("null_nb_film", dict(n=2, nbs=[nb[0], with_film(1, 1, None)])), ("null_nb_albedo", dict(n=2, nbs=[nb[0], with_film(1, 2, None)])),
             ("same_films", dict(o=even)), ("albedo_is_even", dict(al=even)), ("albedo_is_scratch", dict(al=scratch)),
             ("nb_same_films", dict(nbs=[with_film(0, 1, nb[0][0])])), ("nb_albedo_is_its_film", dict(nbs=[with_film(0, 2, nb[0][0])])),
             ("centre_film_twice", dict(nbs=[with_film(0, 0, even)])), ("centre_albedo_twice", dict(nbs=[with_film(0, 2, alb)])),
             ("nb_albedo_twice", dict(n=2, nbs=[nb[0], with_film(1, 2, nb[0][2])])),
             ("scratch_is_even", dict(s=even)), ("scratch_is_nb_film", dict(s=nb[0][1])), ("scratch_is_nb_albedo", dict(s=nb[0][2])),
             ("misaligned_even", dict(e=even + 4)), ("misaligned_albedo", dict(al=alb + 4)), ("misaligned_nb", dict(nbs=[with_film(0, 0, nb[0][0] + 8)])),
             ("misaligned_nb_albedo", dict(nbs=[with_film(0, 2, nb[0][2] + 8)])), ("misaligned_scratch", dict(s=scratch + 12))]
    one_out = [("null_out", dict(out_=None)), ("out_is_even", dict(out_=even)), ("out_is_albedo", dict(out_=alb)), ("out_is_nb_film", dict(out_=nb[0][1])),
               ("out_is_nb_albedo", dict(out_=nb[0][2])), ("out_is_scratch", dict(out_=scratch)), ("misaligned_out", dict(out_=out + 4))]
    cases = {
        "halves": (halves, first + [("null_fa", dict(a=None)), ("null_fb", dict(b=None)), ("fa_is_fb", dict(b=fa)), ("fa_is_even", dict(a=even)),
                                    ("fa_is_albedo", dict(a=alb)), ("fb_is_nb_film", dict(b=nb[0][0])), ("fb_is_nb_albedo", dict(b=nb[0][2])),
                                    ("fa_is_scratch", dict(a=scratch)), ("misaligned_fa", dict(a=fa + 4)), ("misaligned_fb", dict(b=fb + 8))]),
        "guided": (guided, first + one_out + [("null_guide_a", dict(ga_=None)), ("null_guide_b", dict(gb_=None)), ("null_nb_guide_a_array", dict(na=None)),
                                              ("null_nb_guide_b_array", dict(nb_=None)), ("null_nb_guide", dict(nbs=[with_film(0, 4, None)])),
                                              ("same_guides", dict(gb_=ga)), ("nb_same_guides", dict(nbs=[with_film(0, 4, nb[0][3])])),
                                              ("guide_is_its_values", dict(ga_=even, gb_=odd)), ("nb_guide_is_its_values", dict(nbs=[with_film(0, 3, nb[0][0])])),
                                              ("guide_is_albedo", dict(ga_=alb)), ("out_is_guide", dict(out_=gb)), ("out_is_nb_guide", dict(out_=nb[0][4])),
                                              ("scratch_is_guide", dict(s=ga)), ("scratch_is_nb_guide", dict(s=nb[0][3])), ("misaligned_guide", dict(ga_=ga + 4)),
                                              ("misaligned_nb_guide", dict(nbs=[with_film(0, 4, nb[0][4] + 8)]))]),
        "two_pass": (two_pass, first + one_out + [("r2_0", dict(r2=0, rt2=0)), ("r2_11", dict(r2=11)), ("rt2_0", dict(rt2=0)), ("rt2_above_r2", dict(r2=3, rt2=4)),
                                                  ("f2_4", dict(f2=4)), ("k2_0", dict(k2=0.0)), ("k2_neg", dict(k2=-1.0)), ("k2_nan", dict(k2=nan)),
                                                  ("k2_inf", dict(k2=inf))]),
    }
    mark("refused")
    for call_name, (fn, cs) in cases.items():
        for name, kw in cs:
            rc = fn(**kw)
            print("CASE", call_name, name, rc, "|", lib.tray_last_error().decode())
    small = dict(w=1, h=1, n=0, ne=None, no=None, nal=None, r=1, rt=1, f=0)
    for call_name, fn, kw in (("halves", halves, small), ("guided", guided, dict(small, na=None, nb_=None)), ("two_pass", two_pass, dict(small, r2=1, rt2=1, f2=0))):
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
    films = [np.ones((H, W, 4), np.float32) for _ in range(15)]
    pairs = [(films[0], films[1]), (films[2], films[3]), (films[4], films[5])]
    guides = [(films[6], films[7]), (films[8], films[9]), (films[10], films[11])]
    albedos = films[12:15]
    for kw in (dict(), dict(passes=2), dict(passes=2, radius2=3, radius_t2=2, patch2=0, k2=0.5), dict(passes=1)):
        mark("demodulated")
        o = hip.denoise_temporal_demodulated(pairs, albedos, 1, **kw)
        print("OUT", type(o).__name__, o.shape, o.dtype)
    mark("one_frame")
    hip.denoise_temporal_demodulated(pairs[:1], albedos[:1], 0)
    mark("halves")
    o = hip.denoise_temporal_demodulated_halves(pairs, albedos, 1)
    print("HALVES", type(o).__name__, len(o), type(o[0]).__name__, o[0].shape, o[1].dtype)
    mark("guided")
    o = hip.denoise_temporal_demodulated_guided(pairs, albedos, guides, 1)
    print("OUT", type(o).__name__, o.shape, o.dtype)
    mark("tensors")
    t = lambda prs: [(Tensor(a), Tensor(b)) for a, b in prs]
    ta = [Tensor(a) for a in albedos]
    print("TENSORS", type(hip.denoise_temporal_demodulated(t(pairs), ta, 1)).__name__, type(hip.denoise_temporal_demodulated_halves(t(pairs), ta, 1)[1]).__name__,
          type(hip.denoise_temporal_demodulated_guided(t(pairs), ta, t(guides), 1)).__name__)
    # the existing entry points' defaults
    mark("existing_temporal")
    hip.denoise_temporal(pairs, 1)
    mark("existing_albedos")
    hip.denoise_temporal(pairs, 1, albedos=albedos)
    mark("existing_two_pass")
    hip.denoise_temporal(pairs, 1, passes=2)
    mark("existing_halves")
    hip.denoise_temporal_halves(pairs, 1)
    mark("existing_guided")
    hip.denoise_temporal_guided(pairs, guides, 1)
    mark("refused")
    for fn in (lambda: hip.denoise_temporal_demodulated(pairs, albedos[:2], 1), lambda: hip.denoise_temporal_demodulated(pairs, albedos, 1, passes=3),
               lambda: hip.denoise_temporal_demodulated(pairs, ta, 1), lambda: hip.denoise_temporal_demodulated_guided(pairs, albedos, guides[:2], 1),
               lambda: hip.denoise_temporal_demodulated_halves(pairs, albedos, 3),
               lambda: hip.denoise_temporal(pairs, 1, passes=2, albedos=albedos)):
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
    first_hit = hip.render_first_hit_device
    def spy(scene_, frame, select_blocks, spp_, rng, *a, **kw):
        print("ALBEDO", int(frame), tuple(int(v) for v in rng), int(spp_))
        return first_hit(scene_, frame, select_blocks, spp_, rng, *a, **kw)
    hip.render_first_hit_device = spy
    for kw in (dict(), dict(feature_spp=4, radius2=3, radius_t2=2, patch2=0), dict(passes=1)):
        mark("demodulated_sequence")
        Tensor.count = 0
        for frame, img in hip.render_sequence_demodulated(scene, cfg, range(4), reach=1, **kw):
            print("FRAME", frame, img.shape, img.dtype)
        print("FILMS", Tensor.count)
    for kw in (dict(), dict(demodulate=True), dict(passes=2)):
        mark("existing_sequence")
        for frame, img in hip.render_sequence_denoised(scene, cfg, range(4), reach=1, **kw):
            print("FRAME", frame, img.shape, img.dtype)
    mark("refused")
    for fn in (lambda: hip.render_sequence_demodulated(scene, cfg, range(4), reach=1, feature_spp=0),
               lambda: hip.render_sequence_demodulated(scene, cfg, range(4), reach=5),
               lambda: hip.render_sequence_denoised(scene, cfg, range(4), reach=1, passes=2, demodulate=True)):
        try:
            list(fn())
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


def prepare(w, h):
    """tray_denoise_device's two preparing launches (a guide's, a pilot's), streams cut off"""
    return [("prepare", 0, PX(w, h), 256), ("prepare", 1, PX(w, h), 256)]


def values(w, h):
    """the two preparing launches of a frame's demodulated values: k_tdm_prepare and this library's own k_dn_prepare<1>"""
    return [("tdm_prepare", -1, PX(w, h), 256), ("tdm_variance", 1, PX(w, h), 256)]


def halves_call(w, h, n, f=3):
    """the 3 (N + 1) launches of tray_denoise_temporal_demodulated_halves_device"""
    return (values(w, h) + [("t2p_halves", f, TILES(w, h), 512)]) * (n + 1)


def guided_call(w, h, n, f=1):
    """the 5 (N + 1) launches of tray_denoise_temporal_demodulated_guided_device: the values' preparing ones, the guide's, the pass"""
    return (values(w, h) + prepare(w, h) + [("td2_guided", f, TILES(w, h), 512)]) * (n + 1)


def two_pass_call(w, h, n, f=3, f2=1):
    """the 9 N + 6 launches of tray_denoise_temporal_demodulated_two_pass_device"""
    guided = [("td2_guided", f2, TILES(w, h), 512)]
    return halves_call(w, h, n, f) + prepare(w, h) + guided + (values(w, h) + [("halves", f, TILES(w, h), 512)] + prepare(w, h) + guided) * n


def temporal_call(w, h, n):
    """tray_denoise_temporal_device, as tests/test_temporal_stub.py has it"""
    return (prepare(w, h) + [("pass", -1, TILES(w, h), 512)]) * (n + 1)


def tdm_call(w, h, n, f=3):
    """tray_denoise_temporal_demodulated_device, as tests/test_tdemod_stub.py has it"""
    return (values(w, h) + [("tdm_pass", f, TILES(w, h), 512)]) * (n + 1)


def t2_halves_call(w, h, n, f=3):
    """tray_denoise_temporal_halves_device, _guided_device and _two_pass_device, as tests/test_temporal2_stub.py has them"""
    return (prepare(w, h) + [("t2p_halves", f, TILES(w, h), 512)]) * (n + 1)


def t2_guided_call(w, h, n, f=1):
    return (prepare(w, h) * 2 + [("t2p_guided", f, TILES(w, h), 512)]) * (n + 1)


def t2_single_halves(w, h, f=3):
    return prepare(w, h) + [("halves", f, TILES(w, h), 512)]


def t2_two_pass_call(w, h, n, f=3, f2=1):
    guided = [("t2p_guided", f2, TILES(w, h), 512)]
    return t2_halves_call(w, h, n, f) + prepare(w, h) + guided + (t2_single_halves(w, h, f) + prepare(w, h) + guided) * n


CALLS = {"halves": halves_call, "guided": guided_call, "two_pass": two_pass_call}
COUNT = {"halves": lambda n: 3 * (n + 1), "guided": lambda n: 5 * (n + 1), "two_pass": lambda n: 9 * n + 6}
PREFIX = {c: f"tray_denoise_temporal_demodulated_{c}_device" for c in CALLS}


def test_arguments_are_checked_before_any_device_call(host_calls, tmp_path):
    out, log = run(host_calls, tmp_path, "errors")
    cases = [l for l in out.splitlines() if l.startswith("CASE")]
    assert [sum(l.split()[1] == c for l in cases) for c in ("halves", "guided", "two_pass")] == [47, 60, 53], out
    for l in cases:
        head, _, text = l.partition("|")
        _, call, name, rc = head.split()
        assert rc == "-1", (call, name, rc)   # TRAY_E_INVALID
        assert text.strip().startswith(PREFIX[call]) and len(text.strip()) > len(PREFIX[call]) + 10, (call, name, text)
    assert [l.split()[2] for l in out.splitlines() if l.startswith("OK")] == ["0"] * 3, out
    ph = phases(log)
    assert [n for n, _ in ph] == ["refused", "accepted_halves", "accepted_guided", "accepted_two_pass"]
    assert ph[0][1] == [], ph[0][1]   # no launch, no wait, no copy, no fill
    # only the valid calls launched anything: a 1 x 1 film without neighbours is one block of each kernel
    for (name, lines), want in zip(ph[1:], (halves_call(1, 1, 0, 0), guided_call(1, 1, 0, 0), two_pass_call(1, 1, 0, 0, 0))):
        assert [e[:4] for e in launches(lines)] == want and len(lines) == len(want), (name, lines)


def test_scratch_bytes(stub, tmp_path):
    out, _ = run(stub, tmp_path, "launches")
    px, big = 70 * 40, 65535 * 65535
    # the two-pass temporal calls': fixed per pixel whatever N is; no 32-bit overflow
    assert f"SCRATCH {px * 128} {px * 176} {px * 256} 0 0 0 {big * 128} {big * 176} {big * 256}" in out, out


def test_each_call_launches_what_the_header_states_in_order_and_nothing_between(host_calls, tmp_path):
    out, log = run(host_calls, tmp_path, "launches")
    assert out.count("RC ") == 12 and all(l.split()[3] == "0" for l in out.splitlines() if l.startswith("RC ")) and "RC_F 0 0 0" in out, out
    ph = phases(log)
    assert [n for n, _ in ph] == [f"{c}_{n}" for c in CALLS for n in (0, 1, 2, 8)] + ["other_patches"]
    for (name, lines), (c, n) in zip(ph, [(c, n) for c in CALLS for n in (0, 1, 2, 8)]):
        ev = launches(lines)
        assert [e[:4] for e in ev] == CALLS[c](70, 40, n), (name, ev)
        assert len(lines) == len(ev) == COUNT[c](n), (name, [l for l in lines if l.startswith("host")])   # no wait, copy or fill, and nothing else
        assert all(e[4] == "0x5150" for e in ev), (name, ev)
        # this library's kernels are plain launch lines: under no other add-on library's prefix
        own = [l for l in lines if "k_tdm_prepare" in l or "k_td2_guided_pass" in l]
        assert own and all(l.startswith("launch") for l in own), (name, own)
    lines = ph[-1][1]
    assert lines[-1] == "host call=hipDeviceSynchronize", lines[-3:]   # the driver's own wait after the last call
    ev = launches(lines[:-1])
    assert [e[:4] for e in ev] == halves_call(33, 17, 2, 1) + guided_call(33, 17, 2, 0) + two_pass_call(33, 17, 2, 2, 0), ev
    assert len(lines) - 1 == len(ev)


def test_python_entry_points_and_the_existing_ones_defaults(stub, tmp_path):
    out, log = run(stub, tmp_path, "python")
    assert out.count("OUT ndarray (40, 70, 4) float32") == 5, out
    assert "HALVES tuple 2 ndarray (40, 70, 4) float32" in out and "TENSORS Tensor Tensor Tensor" in out, out
    refused = [l for l in out.splitlines() if l.startswith("REFUSED")]
    assert [l.split()[1] for l in refused] == ["ValueError", "ValueError", "TypeError", "ValueError", "ValueError", "ValueError"], out
    assert "passes must be 1 or 2" in refused[1] and "denoise_temporal: passes=2" in refused[5], out   # the existing refusal stays
    ph = [(name, [e[:4] for e in launches(lines)], len(lines)) for name, lines in phases(log)]
    assert [n for n, _, _ in ph] == ["demodulated"] * 4 + ["one_frame", "halves", "guided", "tensors", "existing_temporal", "existing_albedos",
                                                           "existing_two_pass", "existing_halves", "existing_guided", "refused"]
    assert ph[0][1] == ph[1][1] == two_pass_call(70, 40, 2) and ph[0][2] == 24   # passes=2 is the default
    assert ph[2][1] == two_pass_call(70, 40, 2, 3, 0)
    assert ph[3][1] == tdm_call(70, 40, 2) and ph[3][2] == 9   # passes=1: the existing demodulated temporal call
    assert ph[4][1] == two_pass_call(70, 40, 0)
    assert ph[5][1] == halves_call(70, 40, 2)
    assert ph[6][1] == guided_call(70, 40, 2)
    assert ph[7][1] == two_pass_call(70, 40, 2) + halves_call(70, 40, 2) + guided_call(70, 40, 2)
    # the existing entry points launch what tests/test_temporal_stub.py, test_tdemod_stub.py and test_temporal2_stub.py expect
    assert ph[8][1] == temporal_call(70, 40, 2) and ph[8][2] == 9
    assert ph[9][1] == tdm_call(70, 40, 2) and ph[9][2] == 9
    assert ph[10][1] == t2_two_pass_call(70, 40, 2) and ph[10][2] == 24
    assert ph[11][1] == t2_halves_call(70, 40, 2)
    assert ph[12][1] == t2_guided_call(70, 40, 2)
    assert ph[13][1] == [] and ph[13][2] == 0


def test_a_sequence_computes_every_frames_own_halves_and_albedo_once_and_the_existing_sequences_launch_what_they_did(stub, tmp_path):
    out, log = run(stub, tmp_path, "sequence")
    blocks = out.split("FILMS")
    assert len(blocks) == 4
    for b in blocks[:3]:
        assert [l for l in b.splitlines() if l.startswith("FRAME")] == [f"FRAME {f} (48, 64, 4) float32" for f in range(4)], out
    albedo = lambda b: sorted(l for l in b.splitlines() if l.startswith("ALBEDO"))
    assert albedo(blocks[0]) == [f"ALBEDO {f} (0, 16) 16" for f in range(4)]   # each frame's exactly once
    assert albedo(blocks[1]) == [f"ALBEDO {f} (0, 4) 16" for f in range(4)]
    # 5 (2 reach + 1) films, rendered into again, one normal / depth pair, one pair for the centre's halves: 10 reach + 9; passes=1: the existing 11
    assert [b.split()[0] for b in blocks[1:]] == ["19", "19", "11"], out
    refused = [l for l in out.splitlines() if l.startswith("REFUSED")]
    assert len(refused) == 3 and "feature_spp must lie in [1, 16]" in refused[0] and "reach" in refused[1], out
    assert "render_sequence_denoised: passes=2" in refused[2], out   # the existing refusal stays
    ph = phases(log)
    assert [n for n, _ in ph] == ["one_range"] + ["demodulated_sequence"] * 3 + ["existing_sequence"] * 3 + ["refused"]
    (one_range,), = [launches(ph[0][1])]
    assert one_range[0] == "other"
    on_stream = lambda events: [e + ("0x5150",) for e in events]
    render = [one_range] * 2   # a frame's two range launches
    feat = render + [("first_hit", -1, N_TILES, 256, "0x5150")]   # ... then the frame's one first-hit launch
    for (_, lines), f2 in zip(ph[1:3], (1, 0)):
        ev = launches(lines)
        own = feat + on_stream(halves_call(64, 48, 0))   # a frame is rendered, then its own demodulated halves are filtered: once
        frame = lambda n: on_stream(halves_call(64, 48, n) + guided_call(64, 48, n, f2))
        assert ev == own * 2 + frame(1) + own + frame(2) + own + frame(2) + frame(1), ev
        assert sum(e[0] == "first_hit" for e in ev) == 4 and len(lines) == len(ev)
        assert sum(e[0] == "t2p_halves" for e in ev) == 4 + (2 + 3 + 3 + 2)   # four frames' own halves, and the centres' over their windows
    # passes=1 and render_sequence_denoised(demodulate=True): tests/test_tdemod_stub.py's expectation
    frame = lambda n: on_stream(tdm_call(64, 48, n))
    demod = feat * 2 + frame(1) + feat + frame(2) + feat + frame(2) + frame(1)
    assert launches(ph[3][1]) == demod and launches(ph[5][1]) == demod
    # render_sequence_denoised(): tests/test_temporal_stub.py's; (passes=2): tests/test_temporal2_stub.py's
    frame = lambda n: on_stream(temporal_call(64, 48, n))
    assert launches(ph[4][1]) == render * 2 + frame(1) + render + frame(2) + render + frame(2) + frame(1)
    own = render + on_stream(t2_single_halves(64, 48))
    frame = lambda n: on_stream(t2_halves_call(64, 48, n) + t2_guided_call(64, 48, n))
    assert launches(ph[6][1]) == own * 2 + frame(1) + own + frame(2) + own + frame(2) + frame(1)
    assert ph[7][1] == []
