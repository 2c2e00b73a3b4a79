"""The guided filter of tray_denoise_guided_device and the two-pass call tray_denoise_two_pass_device (include/trayhip.h) as numpy statements, typed:
guided(E, O, GA, GB, r, f, k, F) and two_pass(E, O, r, f, k, r2, f2, k2, F) evaluate them in F = np.float32 (the arithmetic the kernels do, in
the order of summation the header defines) or F = np.float64 (what the tests compare with). Built from _denoise_ref's shift, box and resolve;
with the films as their own guide, guided() is _denoise_ref.denoise, operation for operation. Also the bar of the comparisons, the loader of the
host emulation (tests/emu/emu_guided.cpp) with its guarded calls, the GPU tests' calls between guard bytes (torch is imported there, where a
GPU is used), and the parser of the stand-in runtime's log for the stub tests."""
import ctypes as C
import functools
import os

import numpy as np

import tray_rust_amd as T
import _denoise_ref as D
import _emu as E
from _denoise_ref import F32, F64, EPS, box, resolve, shift

GUARD = 64   # floats / bytes around every buffer the emulated kernels write
DEFAULTS2 = (5, 1, 1.0)   # TRAY_DENOISE_RADIUS2, _PATCH2, _K2


def records(even, odd, F):
    """(valid as F, a, b, V) of one pair of films: _denoise_ref.denoise's first lines"""
    valid, a, b = resolve(even, odd, F)
    vm = valid.astype(F)
    v = ((a - b) * (a - b) * F(0.5)).astype(F)
    cnt = box(vm, 1)
    with np.errstate(all="ignore"):
        V = np.where(cnt[..., None] > 0, box(v, 1) / np.maximum(cnt, F(1))[..., None], F(0)).astype(F)
    return vm, a, b, V


def halves(even, odd, ga_film, gb_film, r, f, k, F=F64):
    """(A, B, wA, wB) of the guided filter in F: A = the even film's colours under the weights of guide b, B the other way round, (h, w, 3) each;
    wA / wB: where the denominators are positive. k is the float32 the ABI takes."""
    vm, a, b, _ = records(even, odd, F)
    gvm, ga, gb, Vg = records(ga_film, gb_film, F)
    k2 = F(F32(k)) * F(F32(k))
    eps = F(F32(EPS))
    # both halves in one walk over the offsets -- weights from gb applied to a, weights from ga applied to b --: they share pair and its patch sum,
    # and the three patch sums go through one box() as three channels (the same sums, element for element, as three calls)
    num = [np.zeros_like(a), np.zeros_like(a)]
    den = [np.zeros(a.shape[:2], F), np.zeros(a.shape[:2], F)]
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            Vq, gq, mq = shift(Vg, dy, dx), shift(gvm, dy, dx), shift(vm, dy, dx)
            pair = gvm * gq   # p' and q' valid in the guide, both inside
            with np.errstate(all="ignore"):
                ts = []
                for x in (gb, ga):
                    diff = x - shift(x, dy, dx)
                    t = (diff * diff - (Vg + np.minimum(Vg, Vq))) / (eps + k2 * (Vg + Vq))
                    ts.append((t.sum(-1) * pair).astype(F))
                sums = box(np.stack(ts + [pair], -1), f)
                n = sums[..., 2]
                for i, y in enumerate((a, b)):
                    d2 = np.where(n > 0, sums[..., i] / (F(3) * np.maximum(n, F(1))), F(0))
                    wgt = (np.exp(-np.maximum(d2, F(0))).astype(F) * mq * (n > 0)).astype(F)   # (mq: q valid in the VALUES)
                    num[i] += wgt[..., None] * shift(y, dy, dx)
                    den[i] += wgt
    with np.errstate(all="ignore"):
        outs = [np.where(d[..., None] > 0, m / d[..., None], F(0)).astype(F) for m, d in zip(num, den)]
    have = [d > 0 for d in den]
    return outs[0], outs[1], have[0], have[1]


def guided(even, odd, ga_film, gb_film, r=5, f=1, k=1.0, F=F64):
    """out (h, w, 3) of tray_denoise_guided_device's statement in F"""
    A, B, _, _ = halves(even, odd, ga_film, gb_film, r, f, k, F)
    return ((A + B) * F(0.5)).astype(F)


def pilot(even, odd, r, f, k, F=F64):
    """(fa, fb) of tray_denoise_halves_device's statement as RGBW films in F: weight 1 where a half exists, else 0"""
    A, B, wa, wb = halves(even, odd, even, odd, r, f, k, F)
    return tuple(np.concatenate([x, w[..., None].astype(F)], -1).astype(F) for x, w in ((A, wa), (B, wb)))


def two_pass(even, odd, r=7, f=3, k=0.45, r2=5, f2=1, k2=1.0, F=F64):
    """out (h, w, 3) of tray_denoise_two_pass_device's statement in F: the pilot is computed and used in F"""
    fa, fb = pilot(even, odd, r, f, k, F)
    return guided(even, odd, fa, fb, r2, f2, k2, F)


def bar_of(statement):
    """(want, tolerance, err32, f32) as _denoise_ref.bar, of statement(F): the f64 statement; 4 x the max abs difference of the f32 statement from
    it, plus 1e-7; that difference; the f32 statement"""
    want, f32 = statement(F64), statement(F32)
    err32 = float(np.abs(f32.astype(F64) - want).max())
    return want, 4.0 * err32 + 1e-7, err32, f32


def assert_under_bar(got_rgbw, want_bar, sure, what):
    """_denoise_ref.assert_matches against a bar_of(): got (h, w, 4) against the f64 statement, over the whole image and over the pixels of `sure`
    alone (those whose own weight is 1, so that their denominators are >= 1); weight 1 everywhere; finite; the pixels of rgb == 0 as sets: those
    of the f32 statement exactly, which include those of the f64 one."""
    want, tol, err32, f32 = want_bar
    got = np.asarray(got_rgbw)
    assert np.isfinite(got).all(), f"{what}: non-finite output at {np.argwhere(~np.isfinite(got))[:4].tolist()}"
    assert (got[..., 3] == 1.0).all(), f"{what}: an output weight is not 1"
    diff = np.abs(got[..., :3].astype(F64) - want)
    print(f"{what}: kernels - f64 statement = {diff.max():.3e}, f32 statement - f64 statement = {err32:.3e}, bar {tol:.3e}")
    zero_g, zero_w, zero_64 = (got[..., :3] == 0).all(-1), (f32 == 0).all(-1), (want == 0).all(-1)
    assert (zero_g == zero_w).all(), f"{what}: the pixels with rgb == 0 differ at {np.argwhere(zero_g != zero_w)[:4].tolist()}"
    assert zero_g[zero_64].all(), f"{what}: a pixel the f64 statement leaves 0 is not 0 at {np.argwhere(zero_64 & ~zero_g)[:4].tolist()}"
    assert diff.max() <= tol, f"{what}: {diff.max():.3e} > {tol:.3e} at {np.unravel_index(np.argmax(diff), diff.shape)}"
    if sure.any():
        err_v = float(np.abs(f32.astype(F64) - want)[sure].max())
        print(f"{what}: over the valid pixels {diff[sure].max():.3e}, f32 statement {err_v:.3e}, bar {4.0 * err_v + 1e-7:.3e}")
        assert diff[sure].max() <= 4.0 * err_v + 1e-7, f"{what}: valid pixels: {diff[sure].max():.3e} > {4.0 * err_v + 1e-7:.3e}"
    return float(diff.max()), err32


def sure_pixels(even, odd, ga_film, gb_film):
    """the pixels valid in the values and in the guide: t(p', p') <= 0 and pair(0) = 1, so their own weight is 1 in both halves"""
    return resolve(even, odd)[0] & resolve(ga_film, gb_film)[0]


def assert_guided(got, even, odd, ga_film, gb_film, r, f, k, what):
    return assert_under_bar(got, bar_of(lambda F: guided(even, odd, ga_film, gb_film, r, f, k, F)), sure_pixels(even, odd, ga_film, gb_film), what)


def assert_two_pass(got, even, odd, r, f, k, r2, f2, k2, what):
    """(a valid pixel's own weight is 1 in the first pass, so the pilot is valid there, and 1 again in the second)"""
    return assert_under_bar(got, bar_of(lambda F: two_pass(even, odd, r, f, k, r2, f2, k2, F)), resolve(even, odd)[0], what)


# ---- the host emulation

@functools.lru_cache(None)
def guided_lib():
    deps = [os.path.join(E.EMU_DIR, x) for x in ("hip_emu.h", "emu_denoise.cpp", "emu_guide.cpp")]
    deps += [os.path.join(E.HIP_DIR, h) for h in ("guided_kernels.h", "guide_kernels.h", "block_compact.h", "denoise_kernels.h", "dev_libm.h")]
    deps += E.denoise_plan_deps()
    h = C.CDLL(E.build("libtrayemu_guided.so", "emu_guided.cpp", deps))
    h.emu_denoise_guided.restype = C.c_int
    h.emu_denoise_guided.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p,
                                     C.c_void_p]
    h.emu_denoise_two_pass.restype = C.c_int
    h.emu_denoise_two_pass.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_float, C.c_uint32, C.c_uint32, C.c_float,
                                       C.c_void_p, C.c_void_p]
    for name in ("emu_guided_scratch_bytes", "emu_two_pass_scratch_bytes"):
        getattr(h, name).restype = C.c_uint64
        getattr(h, name).argtypes = [C.c_uint32, C.c_uint32]
    return h


def _emulated(films, nbytes, call):
    """call(out pointer, scratch pointer) between guard words around the output and a scratch buffer of nbytes; the films are what they were
    afterwards; returns (h, w, 4)"""
    before = [x.copy() for x in films]
    h, w = films[0].shape[:2]
    out = np.full(h * w * 4 + 2 * GUARD, -7.0, F32)
    scratch = np.full(nbytes + 2 * GUARD, 0xA5, np.uint8)
    rc = call(out[GUARD:].ctypes.data, scratch[GUARD:].ctypes.data)
    assert rc == 0, rc
    assert (out[:GUARD] == -7.0).all() and (out[-GUARD:] == -7.0).all(), "a write outside the output"
    assert (scratch[:GUARD] == 0xA5).all() and (scratch[-GUARD:] == 0xA5).all(), "a write outside the scratch buffer"
    assert all((x.view(np.uint32) == y.view(np.uint32)).all() for x, y in zip(films, before)), "a film was written"
    return out[GUARD:-GUARD].reshape(h, w, 4).copy()


def run_guided(emu, even, odd, ga_film, gb_film, r, f, k):
    """the five launches of one tray_denoise_guided_device call in the emulation; the guide may be the films themselves"""
    alias_a, alias_b = ga_film is even, gb_film is odd
    even, odd = np.ascontiguousarray(even, F32), np.ascontiguousarray(odd, F32)
    ga = even if alias_a else np.ascontiguousarray(ga_film, F32)
    gb = odd if alias_b else np.ascontiguousarray(gb_film, F32)
    h, w = even.shape[:2]
    return _emulated([even, odd, ga, gb], int(emu.emu_guided_scratch_bytes(w, h)),
                     lambda out, scr: emu.emu_denoise_guided(w, h, even.ctypes.data, odd.ctypes.data, ga.ctypes.data, gb.ctypes.data, r, f, k, out, scr))


def run_two_pass(emu, even, odd, r, f, k, r2, f2, k2):
    """the six launches of one tray_denoise_two_pass_device call in the emulation"""
    even, odd = np.ascontiguousarray(even, F32), np.ascontiguousarray(odd, F32)
    h, w = even.shape[:2]
    return _emulated([even, odd], int(emu.emu_two_pass_scratch_bytes(w, h)),
                     lambda out, scr: emu.emu_denoise_two_pass(w, h, even.ctypes.data, odd.ctypes.data, r, f, k, r2, f2, k2, out, scr))


# ---- on the GPU

def _guarded(host_films, nbytes, call):
    """call(lib, device films, out pointer, scratch pointer, width, height) with the films uploaded from the host, the output and a scratch buffer
    of nbytes(width, height) between guard bytes, the films unchanged afterwards; returns (h, w, 4)"""
    import torch
    guard = D.GPU_GUARD
    h, w = host_films[0].shape[:2]
    lib = T.lib()
    dev = [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in host_films]
    nb = int(nbytes(lib)(w, h))
    scr = torch.full((nb + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((w * h * 16 + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    T.check(lib.tray_init(0))
    T.check(call(lib, [C.c_void_p(x.data_ptr()) for x in dev], C.c_void_p(out.data_ptr() + guard), C.c_void_p(scr.data_ptr() + guard), w, h))
    torch.cuda.synchronize()
    assert (scr[:guard] == 0xA5).all() and (scr[guard + nb:] == 0xA5).all(), "a write outside the scratch buffer's stated size"
    assert (out[:guard] == 0xA5).all() and (out[guard + w * h * 16:] == 0xA5).all(), "a write outside out_dev"
    for x, y in zip(dev, host_films):
        assert (x.cpu().numpy().view(np.uint32) == np.ascontiguousarray(y).view(np.uint32)).all(), "a film was written"
    return out[guard:guard + w * h * 16].view(torch.float32).reshape(h, w, 4).cpu().numpy(), nb


def guided_guarded(even, odd, ga_film, gb_film, r, f, k, alias=False):
    """one tray_denoise_guided_device call; alias: the guide pointers are the films' (ga_film / gb_film are not uploaded)"""
    def call(lib, d, out, scr, w, h):
        ga, gb = (d[0], d[1]) if alias else (d[2], d[3])
        return lib.tray_denoise_guided_device(w, h, d[0], d[1], ga, gb, r, f, k, out, scr, None)
    out, nb = _guarded([even, odd] if alias else [even, odd, ga_film, gb_film], lambda lib: lib.tray_denoise_guided_scratch_bytes, call)
    assert nb == 96 * even.shape[0] * even.shape[1]
    return out


def two_pass_guarded(even, odd, r, f, k, r2, f2, k2):
    """one tray_denoise_two_pass_device call"""
    out, nb = _guarded([even, odd], lambda lib: lib.tray_denoise_two_pass_scratch_bytes,
                       lambda lib, d, out, scr, w, h: lib.tray_denoise_two_pass_device(w, h, d[0], d[1], r, f, k, r2, f2, k2, out, scr, None))
    assert nb == 128 * even.shape[0] * even.shape[1]
    return out


# ---- the stand-in runtime's log (tests/stubs/fakehip.c, tests/_stub.py)

def launches(log):
    """every launch of a log written without FAKEHIP_TILE_KERNEL, in order, as (name, template argument, grid, block, stream): "prepare" (its pass) and
    "filter" (its patch) per kernel of libtrayhip_denoise.so; "halves" (its patch) per k_dn_filter_halves of libtrayhip_guide.so; "guided" (its patch)
    per k_gdn_filter -- the stand-in runtime tells the add-on libraries by their file names, and libtrayhip_guided.so's begins with
    libtrayhip_guide.so's, so its launches are logged with that library's, kernel symbol and all --; ("other", -1, ...) per plain launch line"""
    from _stub import events, kv
    out = []
    named = iter(e for e in events(log) if e[0] in ("denoise", "guide"))
    for l in log:
        if l.startswith(("denoise", "guide")):
            e = next(named)
            name = "halves" if e[1] == "k_dn_filter_halves" else "guided" if "k_gdn_filter" in e[1] else e[1]
            out.append((name,) + e[2:])
        elif l.startswith("launch"):
            n = kv(l)
            out.append(("other", -1, int(n["grid"]), int(n["block"]), n["stream"]))
    return out
