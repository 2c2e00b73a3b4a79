"""What the tests of tray_denoise_temporal_halves_device, tray_denoise_temporal_guided_device and tray_denoise_temporal_two_pass_device share
(include/trayhip.h states the three calls): their numpy statements, typed -- F = np.float32 is the arithmetic the kernels do, in the header's
order of summation, F = np.float64 what the tests compare with --, their bars (_guided_ref.bar_of: 4 x (f32 statement - f64 statement) + 1e-7,
over the whole image and over the centre's valid pixels), the range property over all windows, the loader of the host emulation
(tests/emu/emu_temporal2.cpp) with its guarded calls, the GPU tests' calls between guard bytes (torch is imported there, where a GPU is used),
and the parser of the stand-in runtime's log for the stub tests.

`frames` is a list of (even, odd) RGBW film pairs, frames[0] the centre; `guides` a list of (guide_a, guide_b) pairs, one per frame. halves() is
the one walk over all frames' windows: with the frames as their own guides it is _temporal_ref.temporal, with one frame _guided_ref.halves,
operation for operation (tests/test_temporal2_emu.py compares the f32 values exactly)."""
import ctypes as C
import functools
import os

import numpy as np

import tray_rust_amd as T
import _denoise_ref as D
import _emu as E
import _guided_ref as G
import _temporal_ref as TR
from _denoise_ref import F32, F64, EPS, box, resolve, shift
from _guided_ref import bar_of

GUARD = TR.GUARD
DEFAULTS2 = (5, 3, 1, 1.0)   # TRAY_DENOISE_RADIUS2, _RADIUS_T2, _PATCH2, _K2


# ---- the statements

def halves(frames, guides, r, rt, f, k, F=F64):
    """(A, B, wA, wB) of tray_denoise_temporal_guided_device's statement in F: A = the even films' colours under the weights of the guides' b, B the
    other way round, (h, w, 3) each; wA / wB: where the denominators are positive. k is the float32 the ABI takes. The sums run over frame 0
    (radius r) first, then over frames 1 ... N (radius rt) in list order, within a frame dy outer and dx inner, ascending."""
    vals = [G.records(e, o, F) for e, o in frames]
    gds = [G.records(ga, gb, F) for ga, gb in guides]
    gvm0, ga0, gb0, Vg0 = gds[0]
    k2 = F(F32(k)) * F(F32(k))
    eps = F(F32(EPS))
    num = [np.zeros_like(ga0), np.zeros_like(ga0)]
    den = [np.zeros(ga0.shape[:2], F), np.zeros(ga0.shape[:2], F)]
    for j, ((vmj, aj, bj, _), (gvmj, gaj, gbj, Vgj)) in enumerate(zip(vals, gds)):
        R = r if j == 0 else rt
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                Vq, gq, mq = shift(Vgj, dy, dx), shift(gvmj, dy, dx), shift(vmj, dy, dx)
                pair = gvm0 * gq   # p' valid in the centre's guide, q' valid in frame j's, both inside
                with np.errstate(all="ignore"):
                    ts = []
                    for x0, xj in ((gb0, gbj), (ga0, gaj)):
                        diff = x0 - shift(xj, dy, dx)
                        t = (diff * diff - (Vg0 + np.minimum(Vg0, Vq))) / (eps + k2 * (Vg0 + Vq))
                        ts.append((t.sum(-1) * pair).astype(F))
                    sums = box(np.stack(ts + [pair], -1), f)   # (the three patch sums as three channels: the same sums, element for element)
                    n = sums[..., 2]
                    for i, y in enumerate((aj, bj)):
                        d2 = np.where(n > 0, sums[..., i] / (F(3) * np.maximum(n, F(1))), F(0))
                        wgt = (np.exp(-np.maximum(d2, F(0))).astype(F) * mq * (n > 0)).astype(F)   # (mq: q valid in frame j's VALUES)
                        num[i] += wgt[..., None] * shift(y, dy, dx)
                        den[i] += wgt
    with np.errstate(all="ignore"):
        outs = [np.where(d[..., None] > 0, m / d[..., None], F(0)).astype(F) for m, d in zip(num, den)]
    return outs[0], outs[1], den[0] > 0, den[1] > 0


def _films(A, B, wa, wb, F):
    return tuple(np.concatenate([x, w[..., None].astype(F)], -1).astype(F) for x, w in ((A, wa), (B, wb)))


def temporal_halves(frames, r=7, rt=3, f=3, k=0.45, F=F64):
    """(fa, fb) of tray_denoise_temporal_halves_device's statement as RGBW films in F: weight 1 where a half exists, else 0"""
    return _films(*halves(frames, frames, r, rt, f, k, F), F)


def temporal_guided(frames, guides, r=5, rt=3, f=1, k=1.0, F=F64):
    """out (h, w, 3) of tray_denoise_temporal_guided_device's statement in F"""
    A, B, _, _ = halves(frames, guides, r, rt, f, k, F)
    return ((A + B) * F(0.5)).astype(F)


def pilots(frames, r, rt, f, k, F=F64):
    """the guides of the two-pass call in F: the centre's halves over all frames, every neighbour's own single-frame halves"""
    return [temporal_halves(frames, r, rt, f, k, F)] + [G.pilot(e, o, r, f, k, F) for e, o in frames[1:]]


def two_pass(frames, r=7, rt=3, f=3, k=0.45, r2=5, rt2=3, f2=1, k2=1.0, F=F64, guides=None):
    """out (h, w, 3) of tray_denoise_temporal_two_pass_device's statement in F: the pilots are computed and used in F (guides: pilots() of the same
    arguments, if the caller has them)"""
    return temporal_guided(frames, pilots(frames, r, rt, f, k, F) if guides is None else guides, r2, rt2, f2, k2, F)


def sure_pixels(frames, guides):
    """the pixels valid in the centre's values and in its guide: their own weight is 1 in both halves"""
    return resolve(*frames[0])[0] & resolve(*guides[0])[0]


def assert_halves(got_fa, got_fb, frames, r, rt, f, k, what):
    """(fa, fb) of the kernels against temporal_halves: each half's colours under its own bar_of, over the whole image and over the centre's valid
    pixels; the weights are 0 or 1 and those of the f32 statement; a half without weight is 0"""
    want, f32 = temporal_halves(frames, r, rt, f, k, F64), temporal_halves(frames, r, rt, f, k, F32)
    valid = resolve(*frames[0])[0]
    for name, got, w64, w32 in zip("AB", (np.asarray(got_fa), np.asarray(got_fb)), want, f32):
        assert np.isfinite(got).all(), f"{what} {name}: non-finite output"
        assert (got[..., 3] == w32[..., 3]).all(), f"{what} {name}: the weights differ from the f32 statement's at {np.argwhere(got[..., 3] != w32[..., 3])[:4].tolist()}"
        assert (got[got[..., 3] == 0] == 0).all(), f"{what} {name}: a half without weight is not 0"
        assert (got[..., 3][valid] == 1).all(), f"{what} {name}: a valid pixel of the centre has no weight"
        err = np.abs(w32[..., :3].astype(F64) - w64[..., :3])
        diff = np.abs(got[..., :3].astype(F64) - w64[..., :3])
        tol = 4.0 * float(err.max()) + 1e-7
        print(f"{what} {name}: kernels - f64 statement = {diff.max():.3e}, f32 statement - f64 statement = {err.max():.3e}, bar {tol:.3e}")
        assert diff.max() <= tol, f"{what} {name}: {diff.max():.3e} > {tol:.3e} at {np.unravel_index(np.argmax(diff), diff.shape)}"
        if valid.any():
            tol_v = 4.0 * float(err[valid].max()) + 1e-7
            print(f"{what} {name}: over the valid pixels {diff[valid].max():.3e}, bar {tol_v:.3e}")
            assert diff[valid].max() <= tol_v, f"{what} {name}: valid pixels: {diff[valid].max():.3e} > {tol_v:.3e}"


def assert_guided(got, frames, guides, r, rt, f, k, what):
    return G.assert_under_bar(got, bar_of(lambda F: temporal_guided(frames, guides, r, rt, f, k, F)), sure_pixels(frames, guides), what)


@functools.lru_cache(None)
def _random_pilots(w, h, n, seed, r, rt, f, k):
    """pilots() of random_frames in both types: the second pass's parameters do not enter, so the cases that differ in them share it"""
    frames = TR.random_frames(w, h, n + 1, seed)
    return {F: pilots(frames, r, rt, f, k, F) for F in (F32, F64)}


def assert_two_pass(got, frames, r, rt, f, k, r2, rt2, f2, k2, what, random_key=None):
    """(a valid pixel's own weight is 1 in the first pass, so the centre's pilot is valid there, and 1 again in the second). random_key: (w, h, n,
    seed) if frames is _temporal_ref.random_frames(w, h, n + 1, seed)"""
    cached = _random_pilots(*random_key, r, rt, f, k) if random_key is not None else {}
    return G.assert_under_bar(got, bar_of(lambda F: two_pass(frames, r, rt, f, k, r2, rt2, f2, k2, F, cached.get(F))), resolve(*frames[0])[0], what)


def range_violations(out_rgb, frames, r, rt, where):
    """_temporal_ref.range_violations: the values' range over all frames' windows; `where`: the pixels whose denominators are surely positive"""
    return TR.range_violations(out_rgb, frames, r, rt, where)


def random_guides(w, h, n, seed):
    """n guide pairs that are no film of random_frames(w, h, n, seed): other seeds, other invalid pixels"""
    return TR.random_frames(w, h, n, seed + 5000)


def same_bits(a, b):
    return bool((np.asarray(a).view(np.uint32) == np.asarray(b).view(np.uint32)).all())


# ---- the host emulation

@functools.lru_cache(None)
def temporal2_lib():
    deps = [os.path.join(E.EMU_DIR, x) for x in ("hip_emu.h", "emu_denoise.cpp", "emu_guide.cpp")]
    deps += [os.path.join(E.HIP_DIR, h) for h in ("t2pass_kernels.h", "guide_kernels.h", "block_compact.h", "denoise_kernels.h", "dev_libm.h")]
    deps += E.denoise_plan_deps()
    h = C.CDLL(E.build("libtrayemu_temporal2.so", "emu_temporal2.cpp", deps))
    P = C.POINTER(C.c_void_p)
    u32, f32, ptr = C.c_uint32, C.c_float, C.c_void_p
    h.emu_denoise_temporal_halves.restype = C.c_int
    h.emu_denoise_temporal_halves.argtypes = [u32, u32, ptr, ptr, u32, P, P, u32, u32, u32, f32, ptr, ptr, ptr]
    h.emu_denoise_temporal_guided.restype = C.c_int
    h.emu_denoise_temporal_guided.argtypes = [u32, u32, ptr, ptr, ptr, ptr, u32, P, P, P, P, u32, u32, u32, f32, ptr, ptr]
    h.emu_denoise_temporal_two_pass.restype = C.c_int
    h.emu_denoise_temporal_two_pass.argtypes = [u32, u32, ptr, ptr, u32, P, P, u32, u32, u32, f32, u32, u32, u32, f32, ptr, ptr]
    for name in ("emu_temporal_halves_scratch_bytes", "emu_temporal_guided_scratch_bytes", "emu_temporal_two_pass_scratch_bytes"):
        getattr(h, name).restype = C.c_uint64
        getattr(h, name).argtypes = [u32, u32]
    return h


def _pointers(ptrs):
    return (C.c_void_p * max(len(ptrs), 1))(*ptrs)


def _contiguous(frames, alias_of=None):
    """the films as contiguous f32 arrays; alias_of: the list whose arrays stand in for this one's (the guides ARE the films)"""
    return alias_of if alias_of is not None else [tuple(np.ascontiguousarray(x, F32) for x in fr) for fr in frames]


def _emulated(films, nbytes, n_out, call):
    """call(output pointers, scratch pointer) between guard words around n_out outputs and a scratch buffer of nbytes; the films (a flat list)
    are what they were afterwards; returns the outputs as (h, w, 4)"""
    before = [x.copy() for x in films]
    h, w = films[0].shape[:2]
    outs = [np.full(h * w * 4 + 2 * GUARD, -7.0, F32) for _ in range(n_out)]
    scratch = np.full(nbytes + 2 * GUARD, 0xA5, np.uint8)
    rc = call([o[GUARD:].ctypes.data for o in outs], scratch[GUARD:].ctypes.data)
    assert rc == 0, rc
    for o in outs:
        assert (o[:GUARD] == -7.0).all() and (o[-GUARD:] == -7.0).all(), "a write outside an output"
    assert (scratch[:GUARD] == 0xA5).all() and (scratch[-GUARD:] == 0xA5).all(), "a write outside the scratch buffer"
    assert all(same_bits(x, y) for x, y in zip(films, before)), "a film was written"
    return [o[GUARD:-GUARD].reshape(h, w, 4).copy() for o in outs]


def _arrays(frames):
    """(the centre's pointers, one host array per film of the neighbours)"""
    return [x.ctypes.data for x in frames[0]], [_pointers([fr[i].ctypes.data for fr in frames[1:]]) for i in range(len(frames[0]))]


def run_halves(emu, frames, r, rt, f, k):
    """the 3 (N + 1) launches of one tray_denoise_temporal_halves_device call in the emulation; returns (fa, fb)"""
    frames = _contiguous(frames)
    h, w = frames[0][0].shape[:2]
    nb = int(emu.emu_temporal_halves_scratch_bytes(w, h))
    assert nb == 128 * w * h
    c, nbs = _arrays(frames)
    return tuple(_emulated([x for fr in frames for x in fr], nb, 2,
                           lambda outs, scr: emu.emu_denoise_temporal_halves(w, h, *c, len(frames) - 1, *nbs, r, rt, f, k, *outs, scr)))


def run_guided(emu, frames, guides, r, rt, f, k):
    """the 5 (N + 1) launches of one tray_denoise_temporal_guided_device call in the emulation; `guides is frames`: the guide pointers are the
    films'"""
    fr = _contiguous(frames)
    gd = _contiguous(guides, fr if guides is frames else None)
    h, w = fr[0][0].shape[:2]
    nb = int(emu.emu_temporal_guided_scratch_bytes(w, h))
    assert nb == 176 * w * h
    (e, o), (nbe, nbo) = _arrays(fr)
    (ga, gb), (nga, ngb) = _arrays(gd)
    films = [x for pair in fr + ([] if gd is fr else gd) for x in pair]
    return _emulated(films, nb, 1, lambda outs, scr: emu.emu_denoise_temporal_guided(w, h, e, o, ga, gb, len(fr) - 1, nbe, nbo, nga, ngb, r, rt, f, k,
                                                                                      outs[0], scr))[0]


def run_two_pass(emu, frames, r, rt, f, k, r2, rt2, f2, k2):
    """the 9 N + 6 launches of one tray_denoise_temporal_two_pass_device call in the emulation"""
    frames = _contiguous(frames)
    h, w = frames[0][0].shape[:2]
    nb = int(emu.emu_temporal_two_pass_scratch_bytes(w, h))
    assert nb == 256 * w * h
    c, nbs = _arrays(frames)
    return _emulated([x for fr in frames for x in fr], nb, 1,
                     lambda outs, scr: emu.emu_denoise_temporal_two_pass(w, h, *c, len(frames) - 1, *nbs, r, rt, f, k, r2, rt2, f2, k2, outs[0], scr))[0]


def emulated_composition(emu, frames, r, rt, f, k, r2, rt2, f2, k2):
    """the two-pass call's definition made of emulated calls: the centre's halves over all frames, every neighbour's own halves
    (tray_denoise_halves_device, tests/emu/emu_guide.cpp), the guided call"""
    import _emu_features as EF
    guides = [run_halves(emu, frames, r, rt, f, k)] + [EF.guide_halves(EF.guide_lib(), e, o, r, f, k) for e, o in frames[1:]]
    return run_guided(emu, frames, guides, r2, rt2, f2, k2)


# ---- on the GPU

def _guarded(host_films, scratch_bytes, per_pixel, n_out, call):
    """call(lib, device pointers of host_films, output pointers, scratch pointer, width, height) with the films (a flat list) uploaded from the
    host, n_out outputs and a scratch buffer of scratch_bytes(lib)(width, height) between guard bytes, the films unchanged afterwards; returns
    the outputs as (h, w, 4)"""
    import torch
    guard = D.GPU_GUARD
    h, w = host_films[0].shape[:2]
    lib = T.lib()
    dev = [torch.from_numpy(np.ascontiguousarray(x, F32)).cuda() for x in host_films]
    nb = int(scratch_bytes(lib)(w, h))
    assert nb == per_pixel * w * h
    scr = torch.full((nb + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    outs = [torch.full((w * h * 16 + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(n_out)]
    T.check(lib.tray_init(0))
    T.check(call(lib, [x.data_ptr() for x in dev], [C.c_void_p(o.data_ptr() + guard) for o in outs], C.c_void_p(scr.data_ptr() + guard), w, h))
    torch.cuda.synchronize()
    assert (scr[:guard] == 0xA5).all() and (scr[guard + nb:] == 0xA5).all(), "a write outside the scratch buffer's stated size"
    for o in outs:
        assert (o[:guard] == 0xA5).all() and (o[guard + w * h * 16:] == 0xA5).all(), "a write outside an output"
    for x, y in zip(dev, host_films):
        assert same_bits(x.cpu().numpy(), np.ascontiguousarray(y, F32)), "a film was written"
    return [o[guard:guard + w * h * 16].view(torch.float32).reshape(h, w, 4).cpu().numpy() for o in outs]


def _split(d, n_frames, per_frame):
    """the flat pointer list as (the centre's c_void_p, one host array per film of the neighbours)"""
    fr = [d[per_frame * j:per_frame * (j + 1)] for j in range(n_frames)]
    return [C.c_void_p(p) for p in fr[0]], [_pointers([f[i] for f in fr[1:]]) for i in range(per_frame)]


def halves_guarded(frames, r, rt, f, k):
    """one tray_denoise_temporal_halves_device call; returns (fa, fb)"""
    def call(lib, d, outs, scr, w, h):
        c, nbs = _split(d, len(frames), 2)
        return lib.tray_denoise_temporal_halves_device(w, h, *c, len(frames) - 1, *nbs, r, rt, f, k, *outs, scr, None)
    return tuple(_guarded([x for fr in frames for x in fr], lambda lib: lib.tray_denoise_temporal_halves_scratch_bytes, 128, 2, call))


def guided_guarded(frames, guides, r, rt, f, k):
    """one tray_denoise_temporal_guided_device call; `guides is frames`: the guide pointers are the films' (no guide is uploaded)"""
    alias = guides is frames
    def call(lib, d, outs, scr, w, h):
        (e, o), (nbe, nbo) = _split(d[:2 * len(frames)], len(frames), 2)
        (ga, gb), (nga, ngb) = ((e, o), (nbe, nbo)) if alias else _split(d[2 * len(frames):], len(frames), 2)
        return lib.tray_denoise_temporal_guided_device(w, h, e, o, ga, gb, len(frames) - 1, nbe, nbo, nga, ngb, r, rt, f, k, outs[0], scr, None)
    films = [x for fr in list(frames) + ([] if alias else list(guides)) for x in fr]
    return _guarded(films, lambda lib: lib.tray_denoise_temporal_guided_scratch_bytes, 176, 1, call)[0]


def two_pass_guarded(frames, r, rt, f, k, r2, rt2, f2, k2):
    """one tray_denoise_temporal_two_pass_device call"""
    def call(lib, d, outs, scr, w, h):
        c, nbs = _split(d, len(frames), 2)
        return lib.tray_denoise_temporal_two_pass_device(w, h, *c, len(frames) - 1, *nbs, r, rt, f, k, r2, rt2, f2, k2, outs[0], scr, None)
    return _guarded([x for fr in frames for x in fr], lambda lib: lib.tray_denoise_temporal_two_pass_scratch_bytes, 256, 1, call)[0]


# ---- the stand-in runtime's log (tests/stubs/fakehip.c, tests/_stub.py)

def launches(log):
    """every launch of a log written without FAKEHIP_TILE_KERNEL, in order, as (name, template argument, grid, block, stream): _guided_ref.launches'
    names for the lines of libtrayhip_denoise.so and libtrayhip_guide.so ("prepare", "filter", "halves", "guided"); of the plain launch lines
    (libtrayhip_t2pass.so has no branch in the stand-in runtime) "t2p_halves" (its patch) per k_t2p_halves_pass, "t2p_guided" (its patch) per
    k_t2p_guided_pass, "pass" per other launch of 512 threads (k_tdn_pass, as _temporal_ref.launches tells it) and "other" per other line"""
    from _stub import _template_arg, kv
    named = iter(G.launches([l for l in log if l.startswith(("denoise", "guide"))]))
    out = []
    for l in log:
        if l.startswith(("denoise", "guide")):
            out.append(next(named))
        elif l.startswith("launch"):
            n = kv(l)
            sym = n.get("kernel", "?")
            name, arg = ("t2p_halves", _template_arg(sym)) if "k_t2p_halves_pass" in sym else ("t2p_guided", _template_arg(sym)) if "k_t2p_guided_pass" in sym else \
                        ("pass" if int(n["block"]) == 512 else "other", -1)
            out.append((name, arg, int(n["grid"]), int(n["block"]), n["stream"]))
    return out
