"""What the tests of tray_denoise_temporal_demodulated_device share: the call's numpy statement, typed -- every frame's films divided by the scale
of that frame's albedo film (_first_hit_ref.scale_of), _temporal_ref.temporal of the quotients, times the centre's scale --, its bars, the same
composition around any temporal call (the emulated one, the GPU's) with the two element-wise steps in numpy f32, the loader of the host
emulation (tests/emu/emu_tdemod.cpp) with its guarded call, the GPU tests' one call between guard bytes (torch is imported there, where a GPU
is used), and the parser of the stand-in runtime's log for the stub tests. `frames` is a list of (even, odd, albedo) RGBW films, frames[0] the
centre."""
import ctypes as C
import functools
import json
import os

import numpy as np

import tray_rust_amd as T
import _denoise_ref as D
import _emu as E
import _first_hit_ref as FH
import _temporal_ref as TR
from _denoise_ref import F32, F64

GUARD = TR.GUARD


# ---- the statement

def demodulate(even, odd, albedo, F):
    """(E', O') in F: (x.rgb / s, x.w)"""
    s = FH.scale_of(albedo, F)
    with np.errstate(all="ignore"):
        return tuple(np.concatenate([x.astype(F)[..., :3] / s, x.astype(F)[..., 3:]], -1).astype(F) for x in (even, odd))


def demodulated_frames(frames, F):
    return [demodulate(e, o, a, F) for e, o, a in frames]


def statement(frames, r=7, rt=3, f=3, k=0.45, F=F64):
    """out (h, w, 3) of the call's statement in F"""
    d = TR.temporal(demodulated_frames(frames, F), r, rt, f, k, F)
    return (d * FH.scale_of(frames[0][2], F)).astype(F)


def composed(temporal_call, frames):
    """(h, w, 4): identity (c)'s right-hand side -- numpy-f32 demodulation of every frame, temporal_call(list of (E', O')) -> (h, w, 4), numpy-f32
    remodulation with the centre's scale, weight 1"""
    d = np.asarray(temporal_call(demodulated_frames(frames, F32)), F32)
    s = FH.scale_of(frames[0][2], F32)
    return np.concatenate([(d[..., :3] * s).astype(F32), np.ones_like(d[..., 3:])], -1).astype(F32)


def valid_of(frames):
    """the centre's valid pixels: tray_denoise_device's rule on the f32 quotients"""
    return D.resolve(*demodulate(*frames[0], F32))[0]


def bar(frames, r, rt, f, k):
    """(want, tolerance, err32, tolerance over the centre's valid pixels) as _first_hit_ref.demodulated_bar takes it: the f64 statement; the
    temporal bar's rule -- 4 x the f32 statement's distance from the f64 one, plus 1e-7 -- times the largest s_0; that distance; the same rule
    over the pixels valid in the centre's demodulated films alone, whose denominators are >= 1"""
    want, f32 = (statement(frames, r, rt, f, k, F) for F in (F64, F32))
    err = np.abs(f32.astype(F64) - want)
    s_max = float(FH.scale_of(frames[0][2], F64).max())
    valid = valid_of(frames)
    err_v = float(err[valid].max()) if valid.any() else 0.0
    return want, (4.0 * float(err.max()) + 1e-7) * s_max, float(err.max()), (4.0 * err_v + 1e-7) * s_max


def assert_matches(got_rgbw, frames, r, rt, f, k, what, want_bar=None):
    want, tol, err32, tol_valid = want_bar if want_bar is not None else bar(frames, r, rt, f, k)
    got = np.asarray(got_rgbw)
    assert np.isfinite(got).all() and (got[..., 3] == 1.0).all(), f"{what}: a non-finite word or a weight that is not 1"
    diff = np.abs(got[..., :3].astype(F64) - want)
    valid = valid_of(frames)
    over = float(diff[valid].max()) if valid.any() else 0.0
    print(f"{what}: kernels - f64 statement = {diff.max():.3e}, f32 statement - f64 statement = {err32:.3e}, bar {tol:.3e}; "
          f"over the valid pixels {over:.3e}, bar {tol_valid:.3e}")
    assert diff.max() <= tol, f"{what}: {diff.max():.3e} > {tol:.3e} at {np.unravel_index(np.argmax(diff), diff.shape)}"
    assert over <= tol_valid, f"{what}: valid pixels: {over:.3e} > {tol_valid:.3e}"


def random_frames(w, h, n, seed):
    """n frames of _temporal_ref.random_frames, each with a _first_hit_ref.random_albedo film of a seed of its own"""
    return [(e, o, FH.random_albedo(w, h, seed + 17 * j + 5)) for j, (e, o) in enumerate(TR.random_frames(w, h, n, seed))]


def weightless_albedo(kind, w, h):
    """an albedo film without a valid pixel: s = 1 everywhere"""
    dead = np.ones((h, w, 4), F32)
    if kind == "zero-weight":
        dead[..., 3] = 0.0
    elif kind == "nan":
        dead[:] = np.nan
    else:
        assert kind == "negative-weight", kind
        dead[..., 3] = -2.0
    return dead


def textured_sequence(directory, w, h, spp):
    """Scene.load_file's result for scenes.textured_box as a three-frame sequence (scene_time 1, shutter 0.5): the blink wall's animated image and
    the film strip's movie change from frame to frame; frame 1 is the centre of frames 0 - 2"""
    from tray_rust_amd import scenes
    p = scenes.write_textured_box(directory, width=w, height=h, samples=spp, scene_time=1.0, shutter_size=0.5)
    with open(p) as fh:
        d = json.load(fh)
    d["film"].update({"frames": 3, "end_frame": 2})
    with open(p, "w") as fh:
        json.dump(d, fh)
    return T.Scene.load_file(p)


def same_bits(a, b):
    return bool((np.asarray(a).view(np.uint32) == np.asarray(b).view(np.uint32)).all())


# ---- the host emulation

@functools.lru_cache(None)
def tdemod_lib():
    deps = [os.path.join(E.EMU_DIR, "hip_emu.h")]
    deps += [os.path.join(E.HIP_DIR, h) for h in ("tdemod_kernels.h", "denoise_kernels.h", "dev_libm.h")] + E.denoise_plan_deps()
    h = C.CDLL(E.build("libtrayemu_tdemod.so", "emu_tdemod.cpp", deps))
    P = C.POINTER(C.c_void_p)
    h.emu_denoise_temporal_demodulated.restype = C.c_int
    h.emu_denoise_temporal_demodulated.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, P, P, P, C.c_uint32, C.c_uint32,
                                                   C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]
    h.emu_tdemod_scratch_bytes.restype = C.c_uint64
    h.emu_tdemod_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32]
    return h


def _pointers(ptrs):
    return (C.c_void_p * max(len(ptrs), 1))(*ptrs)


def run(emu, frames, r, rt, f, k):
    """the 3 (N + 1) launches of one call in the emulation; the output and the scratch buffer lie between guard words, and the films are what
    they were afterwards"""
    frames = [tuple(np.ascontiguousarray(x, F32) for x in fr) for fr in frames]
    before = [tuple(x.copy() for x in fr) for fr in frames]
    h, w = frames[0][0].shape[:2]
    out = np.full(h * w * 4 + 2 * GUARD, -7.0, F32)
    nb = int(emu.emu_tdemod_scratch_bytes(w, h))
    assert nb == 128 * w * h
    scratch = np.full(nb + 2 * GUARD, 0xA5, np.uint8)
    nbs = [_pointers([fr[i].ctypes.data for fr in frames[1:]]) for i in range(3)]
    rc = emu.emu_denoise_temporal_demodulated(w, h, *[x.ctypes.data for x in frames[0]], len(frames) - 1, *nbs, r, rt, f, k, out[GUARD:].ctypes.data,
                                              scratch[GUARD:].ctypes.data)
    assert rc == 0, rc
    assert (out[:GUARD] == -7.0).all() and (out[-GUARD:] == -7.0).all(), "a write outside the output"
    assert (scratch[:GUARD] == 0xA5).all() and (scratch[-GUARD:] == 0xA5).all(), "a write outside the scratch buffer"
    for fr, was in zip(frames, before):
        assert all(same_bits(x, y) for x, y in zip(fr, was)), "a film was written"
    return out[GUARD:-GUARD].reshape(h, w, 4).copy()


# ---- on the GPU

def tdemod_guarded(frames, r, rt, f, k):
    """one tray_denoise_temporal_demodulated_device call on films uploaded from the host, its output and scratch buffer between guard bytes, the
    films unchanged afterwards; returns (h, w, 4)"""
    import torch
    guard = D.GPU_GUARD
    h, w = frames[0][0].shape[:2]
    lib = T.lib()
    dev = [tuple(torch.from_numpy(np.ascontiguousarray(x, F32)).cuda() for x in fr) for fr in frames]
    nb = int(lib.tray_denoise_temporal_demodulated_scratch_bytes(w, h))
    assert nb == 128 * w * h
    scr = torch.full((nb + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((w * h * 16 + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    nbs = [_pointers([fr[i].data_ptr() for fr in dev[1:]]) for i in range(3)]
    T.check(lib.tray_init(0))
    T.check(lib.tray_denoise_temporal_demodulated_device(w, h, *[C.c_void_p(x.data_ptr()) for x in dev[0]], len(frames) - 1, *nbs, r, rt, f, k,
                                                         C.c_void_p(out.data_ptr() + guard), C.c_void_p(scr.data_ptr() + guard), None))
    torch.cuda.synchronize()
    assert (scr[:guard] == 0xA5).all() and (scr[guard + nb:] == 0xA5).all(), "a write outside the scratch buffer's stated size"
    assert (out[:guard] == 0xA5).all() and (out[guard + w * h * 16:] == 0xA5).all(), "a write outside out_dev"
    for fr, host in zip(dev, frames):
        assert all(same_bits(x.cpu().numpy(), np.ascontiguousarray(y, F32)) for x, y in zip(fr, host)), "a film was written"
    return out[guard:guard + w * h * 16].view(torch.float32).reshape(h, w, 4).cpu().numpy()


# ---- the stand-in runtime's log (tests/stubs/fakehip.c, tests/_stub.py)

def launches(log):
    """every launch of a log written without FAKEHIP_TILE_KERNEL, in order, as (name, template argument, grid, block, stream): _guided_ref.launches'
    names for the lines of libtrayhip_denoise.so and libtrayhip_guide.so; of the plain launch lines (libtrayhip_tdemod.so has no branch in the
    stand-in runtime) "tdm_prepare" per k_tdm_prepare, "tdm_variance" (1) per k_dn_prepare<1> -- this library's own instance: one of
    libtrayhip_denoise.so's would be a `denoise` line --, "tdm_pass" (its patch) per k_tdm_pass, "first_hit" per k_first_hit_tiles, "pass" per other launch of
    512 threads (k_tdn_pass, as _temporal_ref.launches tells it) and "other" per other line"""
    from _stub import _template_arg, kv
    import _guided_ref as G
    named = iter(G.launches([l for l in log if l.startswith(("denoise", "guide"))]))
    out = []
    for l in log:
        if l.startswith(("denoise", "guide")):
            out.append(next(named))
        elif l.startswith("launch"):
            n = kv(l)
            sym = n.get("kernel", "?")
            name, arg = ("tdm_prepare", -1) if "k_tdm_prepare" in sym else ("tdm_variance", _template_arg(sym)) if "k_dn_prepare" in sym else \
                        ("tdm_pass", _template_arg(sym)) if "k_tdm_pass" in sym else ("first_hit", -1) if "k_first_hit_tiles" in sym else ("pass" if int(n["block"]) == 512 else "other", -1)
            out.append((name, arg, int(n["grid"]), int(n["block"]), n["stream"]))
    return out
