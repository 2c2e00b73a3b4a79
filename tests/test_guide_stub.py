"""tray_denoise_halves_device and tray_render_noise_target_filtered_device through the real library against the stand-in runtime
(tests/stubs/fakehip.c: one log line per launch of libtrayhip_guide.so), as tests/test_denoise_stub.py: every
TRAY_E_INVALID case of include/trayhip.h for both calls, the scratch size, the launches of a halves call, round 0's launch sequence of the
filtered rule (the stand-in block compaction answers "every block", the stand-in tile compaction "no tile": the call ends after round 0), and
tray_render_noise_target_device / tray_denoise_device launching exactly what they launched before."""
import os

from _stub import events as all_events, stub   # (stub: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

DRIVER = r'''
import ctypes as C, os, sys
sys.path.insert(0, %(root)r)
import tray_rust_amd as T
from tray_rust_amd import _lib as L, scenes
lib = T.lib()
mode = %(mode)r
W, H = 64, 48
al = lambda b: (C.addressof(b) + 15) & ~15
films = [C.create_string_buffer(W * H * 16 + 32) for _ in range(5)]
even, odd, fa, fb, out = (al(b) for b in films)
nb_f = int(lib.tray_denoise_scratch_bytes(W, H))
nb_g = int(lib.tray_noise_target_filtered_scratch_bytes(W, H))
print("SCRATCH", nb_f, nb_g)
scr = C.create_string_buffer(nb_g + 32)
scratch = al(scr)
blk = (C.c_uint32 * 8)(0, 1, 2, 3, 4, 5, 0, 0)
def halves(w=W, h=H, e=even, o=odd, r=7, f=3, k=0.45, bl=None, n=0, a=fa, b=fb, s=scratch, stream=None):
    return lib.tray_denoise_halves_device(w, h, e, o, r, f, k, bl, n, a, b, s, stream)
smp, err = (C.c_uint32 * 48)(), (C.c_float * 48)()
def scene_dev():
    d = %(tmp)r
    scenes.write_assets(d, cornell=(W, H, 16))
    scene, rt, spp, fi = T.Scene.load_file(os.path.join(d, "cornell_box.json"))
    return scene, scene.device_scene(0, 0)
def filtered(dev, start=0, count=0, lo=8, hi=64, thr=0.05, e=even, o=odd, r=7, f=3, k=0.45, out_=None, s=scratch, sm=smp, er=err, stream=None):
    return lib.tray_render_noise_target_filtered_device(dev, start, count, lo, hi, thr, 3, e, o, r, f, k, out_, s, sm, er, stream)
if mode == "halves_errors":
    print("CASE init", lib.tray_init(0))
    nan, inf = float("nan"), float("inf")
    for name, kw in [("w0", dict(w=0)), ("h0", dict(h=0)), ("r0", dict(r=0)), ("r11", dict(r=11)), ("f4", dict(f=4)), ("k0", dict(k=0.0)),
                     ("kneg", dict(k=-0.45)), ("knan", dict(k=nan)), ("kinf", dict(k=inf)), ("null_even", dict(e=None)), ("null_odd", dict(o=None)),
                     ("null_fa", dict(a=None)), ("null_fb", dict(b=None)), ("null_scratch", dict(s=None)), ("same_films", dict(o=even)),
                     ("fa_is_even", dict(a=even)), ("fa_is_odd", dict(a=odd)), ("fb_is_even", dict(b=even)), ("fb_is_odd", dict(b=odd)),
                     ("fa_is_fb", dict(b=fa)), ("scratch_is_even", dict(s=even)), ("scratch_is_odd", dict(s=odd)), ("scratch_is_fa", dict(s=fa)),
                     ("scratch_is_fb", dict(s=fb)), ("misaligned_even", dict(e=even + 4)), ("misaligned_odd", dict(o=odd + 8)),
                     ("misaligned_fa", dict(a=fa + 4)), ("misaligned_fb", dict(b=fb + 12)), ("misaligned_scratch", dict(s=scratch + 4)),
                     ("list_too_long", dict(bl=blk, n=7))]:
        print("CASE", name, halves(**kw))
    print("CASE empty_list", halves(bl=blk, n=0))
    print("CASE smallest", halves(w=1, h=1, r=1, f=0))
elif mode == "halves_launches":
    T.check(lib.tray_init(0))
    print("RC", halves(stream=C.c_void_p(0x5150)))
    print("RC_LIST", halves(bl=blk, n=4, r=3, f=1))
    print("RC_EMPTY", halves(bl=blk, n=0))
    print("RC_F0", halves(w=33, h=17, r=1, f=0))
    print("RC_F2", halves(w=1, h=1, r=2, f=2))
elif mode == "filtered_errors":
    scene, dev = scene_dev()
    nan, inf = float("nan"), float("inf")
    for name, kw in [("min1", dict(lo=1)), ("min0", dict(lo=0)), ("min3", dict(lo=3)), ("max12", dict(hi=12)), ("max_below_min", dict(lo=16, hi=8)),
                     ("negative", dict(thr=-0.5)), ("nan", dict(thr=nan)), ("null_even", dict(e=None)), ("null_odd", dict(o=None)),
                     ("same_film", dict(o=even)), ("null_samples", dict(sm=None)), ("null_error", dict(er=None)), ("null_scratch", dict(s=None)),
                     ("r0", dict(r=0)), ("r11", dict(r=11)), ("f4", dict(f=4)), ("k0", dict(k=0.0)), ("kneg", dict(k=-1.0)), ("knan", dict(k=nan)),
                     ("kinf", dict(k=inf)), ("out_is_even", dict(out_=even)), ("out_is_odd", dict(out_=odd)), ("out_is_scratch", dict(out_=scratch)),
                     ("scratch_is_even", dict(s=even)), ("scratch_is_odd", dict(s=odd)), ("misaligned_even", dict(e=even + 4)),
                     ("misaligned_odd", dict(o=odd + 4)), ("misaligned_out", dict(out_=out + 8)), ("misaligned_scratch", dict(s=scratch + 4))]:
        print("CASE", name, filtered(dev, **kw))
    print("CASE null_scene", filtered(None))
    T.check(lib.tray_scene_set_sampler(dev, 1, 1, 1))
    print("CASE uniform", filtered(dev))
    T.check(lib.tray_scene_set_sampler(dev, 2, 4, 16))
    print("CASE adaptive", filtered(dev))
    T.check(lib.tray_scene_set_sampler(dev, 0, 1, 1))
    print("CASE min_equals_max", filtered(dev, lo=16, hi=16, thr=0.0))
elif mode == "round0":
    scene, dev = scene_dev()
    print("RC", filtered(dev, stream=None))
    t = L.TrayKernelTiming()
    print("TIMING", lib.tray_last_timing(dev, C.byref(t)), t.launches)
    print("RC_OUT", filtered(dev, start=5, count=10, lo=2, hi=4, r=3, f=1, out_=out))
    print("TIMING_OUT", lib.tray_last_timing(dev, C.byref(t)), t.launches)
else:
    scene, dev = scene_dev()
    print("RC_NT", lib.tray_render_noise_target_device(dev, 0, 0, 8, 64, 0.05, 3, even, odd, smp, err, None))
    t = L.TrayKernelTiming()
    print("TIMING", lib.tray_last_timing(dev, C.byref(t)), t.launches)
    print("RC_DN", lib.tray_denoise_device(W, H, even, odd, 7, 3, 0.45, out, scratch, None))
print("DONE")
'''


def run(stub, tmp_path, mode):
    out, log = stub(DRIVER % {"root": ROOT, "tmp": str(tmp_path), "mode": mode}, tmp_path, FAKEHIP_DEVICES=1, FAKEHIP_TILE_KERNEL=1)
    assert "DONE" in out.stdout, out.stdout + out.stderr
    return out.stdout, log


PX = lambda w, h: (w * h + 255) // 256
BLOCKS = lambda w, h: ((w + 31) // 32) * ((h + 15) // 16)
NIL = ("(nil)", "0", "0x0")


def cases(out):
    return dict(l.split()[1:] for l in out.splitlines() if l.startswith("CASE"))


def test_halves_arguments_are_checked(stub, tmp_path):
    out, log = run(stub, tmp_path, "halves_errors")
    rc = cases(out)
    assert rc.pop("init") == "0"
    assert rc.pop("smallest") == "0" and rc.pop("empty_list") == "0", out
    assert len(rc) == 30 and all(v == "-1" for v in rc.values()), rc   # TRAY_E_INVALID
    # only the smallest call launched anything (an empty list launches nothing): a 1 x 1 film is one block of each kernel
    ev = all_events(log)
    assert [e[:5] for e in ev] == [("denoise", "prepare", 0, 1, 256), ("denoise", "prepare", 1, 1, 256), ("guide", "k_dn_filter_halves", 0, 1, 512)], ev


def test_scratch_bytes(stub, tmp_path):
    out, _ = run(stub, tmp_path, "halves_launches")
    nb_f, nb_g = (int(v) for v in next(l for l in out.splitlines() if l.startswith("SCRATCH")).split()[1:])
    assert nb_f == 64 * 48 * 48
    assert nb_g == nb_f + 2 * 64 * 48 * 16 + 2 * 4 * BLOCKS(64, 48) + 16   # the filter's records, fa and fb, the flags and the list, the counts


def test_a_halves_call_is_three_launches_on_the_callers_stream(stub, tmp_path):
    out, log = run(stub, tmp_path, "halves_launches")
    for k in ("RC 0", "RC_LIST 0", "RC_EMPTY 0", "RC_F0 0", "RC_F2 0"):
        assert k in out, out
    ev = all_events(log)
    assert [e[:5] for e in ev] == [
        ("denoise", "prepare", 0, PX(64, 48), 256), ("denoise", "prepare", 1, PX(64, 48), 256), ("guide", "k_dn_filter_halves", 3, BLOCKS(64, 48), 512),
        ("denoise", "prepare", 0, PX(64, 48), 256), ("denoise", "prepare", 1, PX(64, 48), 256), ("guide", "k_dn_filter_halves", 1, 4, 512),
        ("denoise", "prepare", 0, PX(33, 17), 256), ("denoise", "prepare", 1, PX(33, 17), 256), ("guide", "k_dn_filter_halves", 0, 4, 512),
        ("denoise", "prepare", 0, 1, 256), ("denoise", "prepare", 1, 1, 256), ("guide", "k_dn_filter_halves", 2, 1, 512)], ev
    assert all(e[5] == "0x5150" for e in ev[:3]) and all(e[5] in NIL for e in ev[3:]), ev


def test_filtered_arguments_are_checked(stub, tmp_path):
    out, log = run(stub, tmp_path, "filtered_errors")
    rc = cases(out)
    assert rc.pop("uniform") == "-4" and rc.pop("adaptive") == "-4", out   # TRAY_E_UNSUPPORTED
    assert rc.pop("min_equals_max") == "0", out
    assert len(rc) == 30 and all(v == "-1" for v in rc.values()), rc
    ev = all_events(log)
    assert ev[:2] == [("guide", "k_guide_mark", -1, 1, 256, ev[0][5]), ("guide", "k_guide_compact", -1, 1, 1024, ev[1][5])]
    assert [e[:3] for e in ev if e[0] == "range"] == [("range", 0, 8), ("range", 8, 16)]   # only the valid call rendered


def round0(w, h, n_tiles, lo, patch, spp, out):
    """the launches of a filtered call that ends after round 0, as all_events reports them (streams cut off)"""
    ev = [("guide", "k_guide_mark", -1, (n_tiles + 255) // 256, 256), ("guide", "k_guide_compact", -1, 1, 1024),
          ("range", 0, lo // 2, n_tiles, spp, n_tiles, 1), ("range", lo // 2, lo, n_tiles, spp, n_tiles, 1),
          ("denoise", "prepare", 0, PX(w, h), 256), ("denoise", "prepare", 1, PX(w, h), 256), ("guide", "k_dn_filter_halves", patch, BLOCKS(w, h), 512),
          ("noise", "error", (n_tiles + 3) // 4, 256), ("noise", "compact", 1, 1024),
          ("guide", "k_guide_mark", -1, (n_tiles + 255) // 256, 256), ("guide", "k_guide_compact", -1, 1, 1024)]
    if out:
        ev += [("denoise", "prepare", 0, PX(w, h), 256), ("denoise", "prepare", 1, PX(w, h), 256), ("denoise", "filter", patch, BLOCKS(w, h), 512)]
    return ev


def test_round_0_of_the_filtered_rule(stub, tmp_path):
    out, log = run(stub, tmp_path, "round0")
    assert "RC 0" in out and "RC_OUT 0" in out, out
    ev = [e[:5] if e[0] in ("guide", "denoise") else e for e in all_events(log)]
    first, second = round0(64, 48, 48, 8, 3, 64, False), round0(64, 48, 10, 2, 1, 4, True)
    assert ev == first + second, ev
    # TrayKernelTiming counts every launch of the call
    assert f"TIMING 0 {len(first)}" in out and f"TIMING_OUT 0 {len(second)}" in out, out


def test_the_existing_calls_launch_what_they_launched_before(stub, tmp_path):
    out, log = run(stub, tmp_path, "renders")
    assert "RC_NT 0" in out and "RC_DN 0" in out and "TIMING 0 4" in out, out
    ev = all_events(log)
    assert not any(e[0] == "guide" for e in ev)
    assert [e[:5] if e[0] == "denoise" else e for e in ev] == [
        ("range", 0, 4, 48, 64, 48, 1), ("range", 4, 8, 48, 64, 48, 1), ("noise", "error", 12, 256), ("noise", "compact", 1, 1024),
        ("denoise", "prepare", 0, PX(64, 48), 256), ("denoise", "prepare", 1, PX(64, 48), 256), ("denoise", "filter", 3, BLOCKS(64, 48), 512)]
