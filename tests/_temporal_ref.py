"""The temporal filter of tray_denoise_temporal_device (include/trayhip.h) as a numpy statement, typed: temporal(frames, r, rt, f, k, F) evaluates
it in F = np.float32 (the arithmetic the kernels do, in the order of summation the header defines) or F = np.float64 (what the tests compare
with). `frames` is a list of (even, odd) RGBW film pairs, frames[0] the centre. Built from _denoise_ref's shift, box and resolve; with one frame
it is _denoise_ref.denoise, operation for operation. Also the bar of the comparisons and the range property over all frames' windows, the
loader of the host emulation (tests/emu/emu_temporal.cpp) with its guarded call, the GPU tests' one call of tray_denoise_temporal_device between
guard bytes (torch is imported there, where a GPU is used), and the parser of the stand-in runtime's log for the stub tests."""
import ctypes as C
import functools
import os

import numpy as np

import tray_rust_amd as T
import _denoise_ref as D
import _emu as E
from _denoise_ref import F32, F64, EPS, box, resolve, shift

GUARD = 64   # floats / bytes around every buffer the emulated kernels write


def records(even, odd, F):
    """(valid as F, a, b, V) of one frame: _denoise_ref.denoise's first lines"""
    valid, a, b = resolve(even, odd, F)
    vm = valid.astype(F)
    v = ((a - b) * (a - b) * F(0.5)).astype(F)
    cnt = box(vm, 1)
    with np.errstate(all="ignore"):
        V = np.where(cnt[..., None] > 0, box(v, 1) / np.maximum(cnt, F(1))[..., None], F(0)).astype(F)
    return vm, a, b, V


def temporal(frames, r=7, rt=3, f=3, k=0.45, F=F64):
    """out (h, w, 3) of the filter in F. k is the float32 the ABI takes. The sums run over frame 0 (radius r) first, then over frames 1 ... N
    (radius rt) in list order, within a frame dy outer and dx inner, ascending."""
    rec = [records(e, o, F) for e, o in frames]
    vm0, V0 = rec[0][0], rec[0][3]
    k2 = F(F32(k)) * F(F32(k))
    eps = F(F32(EPS))
    outs = []
    for xi, yi in ((2, 1), (1, 2)):   # weights from x (b, then a), applied to y
        x0 = rec[0][xi]
        num = np.zeros_like(x0)
        den = np.zeros(x0.shape[:2], F)
        for j, fr in enumerate(rec):
            vmj, xj, yj, Vj = fr[0], fr[xi], fr[yi], fr[3]
            R = r if j == 0 else rt
            for dy in range(-R, R + 1):
                for dx in range(-R, R + 1):
                    xq, Vq, mq = shift(xj, dy, dx), shift(Vj, dy, dx), shift(vmj, dy, dx)
                    pair = vm0 * mq   # p' valid in the centre frame, q' valid in frame j, both inside
                    diff = x0 - xq
                    with np.errstate(all="ignore"):
                        t = (diff * diff - (V0 + np.minimum(V0, Vq))) / (eps + k2 * (V0 + Vq))
                        t = (t.sum(-1) * pair).astype(F)
                        n = box(pair, f)
                        d2 = np.where(n > 0, box(t, f) / (F(3) * np.maximum(n, F(1))), F(0))
                        wgt = (np.exp(-np.maximum(d2, F(0))).astype(F) * mq * (n > 0)).astype(F)
                    num += wgt[..., None] * shift(yj, dy, dx)
                    den += wgt
        with np.errstate(all="ignore"):
            outs.append(np.where(den[..., None] > 0, num / den[..., None], F(0)).astype(F))
    return ((outs[0] + outs[1]) * F(0.5)).astype(F)


def offsets(n_neighbours, r, rt):
    """the window offsets of all frames"""
    return (2 * r + 1) ** 2 + n_neighbours * (2 * rt + 1) ** 2


def bar(frames, r, rt, f, k):
    """(want, tolerance, err32, f32) as _denoise_ref.bar: the f64 statement; 4 x the max abs difference of the f32 statement from it, plus 1e-7;
    that difference; the f32 statement"""
    want = temporal(frames, r, rt, f, k, F64)
    f32 = temporal(frames, r, rt, f, k, F32)
    err32 = float(np.abs(f32.astype(F64) - want).max())
    return want, 4.0 * err32 + 1e-7, err32, f32


def assert_matches(got_rgbw, frames, r, rt, f, k, what, want_bar=None):
    """_denoise_ref.assert_matches for the temporal statement: got (h, w, 4) against the f64 statement under bar(), over the whole image and over
    the centre frame's valid pixels alone (their own weight in frame 0 is 1, so their denominators are >= 1); weight 1 everywhere; finite; the
    pixels of rgb == 0 as sets: those of the f32 statement exactly, which include those of the f64 one. want_bar: bar() of the same input, if
    the caller has it."""
    want, tol, err32, f32 = want_bar if want_bar is not None else bar(frames, r, rt, f, k)
    got = np.asarray(got_rgbw)
    assert np.isfinite(got).all(), f"{what}: non-finite output at {np.argwhere(~np.isfinite(got))[:4].tolist()}"
    assert (got[..., 3] == 1.0).all(), f"{what}: an output weight is not 1"
    diff = np.abs(got[..., :3].astype(F64) - want)
    print(f"{what}: kernels - f64 statement = {diff.max():.3e}, f32 statement - f64 statement = {err32:.3e}, bar {tol:.3e}")
    zero_g, zero_w, zero_64 = (got[..., :3] == 0).all(-1), (f32 == 0).all(-1), (want == 0).all(-1)
    assert (zero_g == zero_w).all(), f"{what}: the pixels with rgb == 0 differ at {np.argwhere(zero_g != zero_w)[:4].tolist()}"
    assert zero_g[zero_64].all(), f"{what}: a pixel the f64 statement leaves 0 is not 0 at {np.argwhere(zero_64 & ~zero_g)[:4].tolist()}"
    assert diff.max() <= tol, f"{what}: {diff.max():.3e} > {tol:.3e} at {np.unravel_index(np.argmax(diff), diff.shape)}"
    valid = resolve(*frames[0])[0]
    if valid.any():
        err_v = float(np.abs(f32.astype(F64) - want)[valid].max())
        print(f"{what}: over the valid pixels {diff[valid].max():.3e}, f32 statement {err_v:.3e}, bar {4.0 * err_v + 1e-7:.3e}")
        assert diff[valid].max() <= 4.0 * err_v + 1e-7, f"{what}: valid pixels: {diff[valid].max():.3e} > {4.0 * err_v + 1e-7:.3e}"
    return float(diff.max()), err32


def range_violations(out_rgb, frames, r, rt, where=None):
    """_denoise_ref.range_violations over the union of all frames' windows: every output channel lies between the minimum and the maximum of that
    channel of a_j and b_j over the valid pixels of the pixel's window in frame 0 (radius r) and in every other frame (radius rt), up to
    (2 * offsets + 4) 2^-24 times the largest magnitude there. Default `where`: the centre frame's valid pixels, whose denominators are >= 1."""
    h, w = frames[0][0].shape[:2]
    slack = (2 * offsets(len(frames) - 1, r, rt) + 4) * 2.0 ** -24
    wlo, whi = np.full((h, w, 3), np.inf), np.full((h, w, 3), -np.inf)
    for j, (even, odd) in enumerate(frames):
        valid, a, b = resolve(even, odd, F32)
        lo = np.where(valid[..., None], np.minimum(a, b), np.inf).astype(F64)
        hi = np.where(valid[..., None], np.maximum(a, b), -np.inf).astype(F64)
        R = r if j == 0 else rt
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                ys0, ys1, xs0, xs1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
                if ys0 < ys1 and xs0 < xs1:
                    wlo[ys0:ys1, xs0:xs1] = np.minimum(wlo[ys0:ys1, xs0:xs1], lo[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx])
                    whi[ys0:ys1, xs0:xs1] = np.maximum(whi[ys0:ys1, xs0:xs1], hi[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx])
    none = ~np.isfinite(wlo)   # no valid pixel in any window: the output is 0
    wlo, whi = np.where(none, 0.0, wlo), np.where(none, 0.0, whi)
    mag = np.maximum(np.abs(wlo), np.abs(whi))
    o = np.asarray(out_rgb, F64)
    bad = (o < wlo - slack * mag) | (o > whi + slack * mag)
    return np.argwhere(bad.any(-1) & (resolve(*frames[0])[0] if where is None else np.asarray(where, bool)))


def random_frames(w, h, n, seed):
    """n film pairs of _denoise_ref.random_films, each of a seed of its own"""
    return [D.random_films(w, h, seed=seed + 101 * j) for j in range(n)]


# ---- the host emulation

@functools.lru_cache(None)
def temporal_lib():
    deps = [os.path.join(E.EMU_DIR, "hip_emu.h"), os.path.join(E.EMU_DIR, "emu_denoise.cpp")]
    deps += [os.path.join(E.HIP_DIR, h) for h in ("temporal_kernels.h", "denoise_kernels.h", "dev_libm.h")] + E.denoise_plan_deps()
    h = C.CDLL(E.build("libtrayemu_temporal.so", "emu_temporal.cpp", deps))
    h.emu_denoise_temporal.restype = C.c_int
    h.emu_denoise_temporal.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.c_uint32,
                                       C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]
    h.emu_temporal_scratch_bytes.restype = C.c_uint64
    h.emu_temporal_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32]
    return h


def _pointers(ptrs):
    return (C.c_void_p * max(len(ptrs), 1))(*ptrs)


def run(emu, frames, r, rt, f, k):
    """the 3 (N + 1) launches of one tray_denoise_temporal_device call in the emulation (frames[0]: the centre); the output and the scratch buffer
    lie between guard words, and the films are what they were afterwards"""
    frames = [tuple(np.ascontiguousarray(x, F32) for x in fr) for fr in frames]
    before = [tuple(x.copy() for x in fr) for fr in frames]
    h, w = frames[0][0].shape[:2]
    out = np.full(h * w * 4 + 2 * GUARD, -7.0, F32)
    nb = int(emu.emu_temporal_scratch_bytes(w, h))
    scratch = np.full(nb + 2 * GUARD, 0xA5, np.uint8)
    nbe, nbo = _pointers([fr[0].ctypes.data for fr in frames[1:]]), _pointers([fr[1].ctypes.data for fr in frames[1:]])
    rc = emu.emu_denoise_temporal(w, h, frames[0][0].ctypes.data, frames[0][1].ctypes.data, len(frames) - 1, nbe, nbo, r, rt, f, k, out[GUARD:].ctypes.data,
                                  scratch[GUARD:].ctypes.data)
    assert rc == 0, rc
    assert (out[:GUARD] == -7.0).all() and (out[-GUARD:] == -7.0).all(), "a write outside the output"
    assert (scratch[:GUARD] == 0xA5).all() and (scratch[-GUARD:] == 0xA5).all(), "a write outside the scratch buffer"
    for fr, was in zip(frames, before):
        assert all((x.view(np.uint32) == y.view(np.uint32)).all() for x, y in zip(fr, was)), "a film was written"
    return out[GUARD:-GUARD].reshape(h, w, 4).copy()


# ---- on the GPU

def temporal_guarded(frames, r, rt, f, k):
    """one tray_denoise_temporal_device call on films uploaded from the host (frames[0]: the centre), its output and scratch buffer between guard
    bytes, the films unchanged afterwards; returns (h, w, 4)"""
    import torch
    guard = D.GPU_GUARD
    h, w = frames[0][0].shape[:2]
    lib = T.lib()
    dev = [tuple(torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in fr) for fr in frames]
    nb = int(lib.tray_denoise_temporal_scratch_bytes(w, h))
    assert nb == 128 * w * h
    scr = torch.full((nb + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((w * h * 16 + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    nbe, nbo = _pointers([fr[0].data_ptr() for fr in dev[1:]]), _pointers([fr[1].data_ptr() for fr in dev[1:]])
    T.check(lib.tray_init(0))
    T.check(lib.tray_denoise_temporal_device(w, h, C.c_void_p(dev[0][0].data_ptr()), C.c_void_p(dev[0][1].data_ptr()), len(frames) - 1, nbe, nbo, r, rt, f, k,
                                             C.c_void_p(out.data_ptr() + guard), C.c_void_p(scr.data_ptr() + guard), None))
    torch.cuda.synchronize()
    assert (scr[:guard] == 0xA5).all() and (scr[guard + nb:] == 0xA5).all(), "a write outside tray_denoise_temporal_scratch_bytes of scratch"
    assert (out[:guard] == 0xA5).all() and (out[guard + w * h * 16:] == 0xA5).all(), "a write outside out_dev"
    for fr, host in zip(dev, frames):
        assert all((x.cpu().numpy().view(np.uint32) == np.ascontiguousarray(y).view(np.uint32)).all() for x, y in zip(fr, host)), "a film was written"
    return out[guard:guard + w * h * 16].view(torch.float32).reshape(h, w, 4).cpu().numpy()


# ---- the stand-in runtime's log (tests/stubs/fakehip.c, tests/_stub.py)

def launches(log):
    """every launch of a log written without FAKEHIP_TILE_KERNEL, in order: ("prepare", pass, grid, block, stream) per k_dn_prepare of
    libtrayhip_denoise.so, ("filter", patch, grid, block, stream) per k_dn_filter, and (the stand-in runtime has no branch for
    libtrayhip_temporal.so: its launches are plain launch lines) ("pass", -1, grid, block, stream) per launch line of 512 threads, which is
    k_tdn_pass's block and no render kernel's, ("other", -1, grid, block, stream) per other launch line"""
    from _stub import events, kv
    out = []
    denoise = iter(e for e in events(log) if e[0] == "denoise")
    for l in log:
        if l.startswith("denoise"):
            out.append(next(denoise)[1:])
        elif l.startswith("launch"):
            n = kv(l)
            out.append(("pass" if int(n["block"]) == 512 else "other", -1, int(n["grid"]), int(n["block"]), n["stream"]))
    return out
