"""What the tests of tray_denoise_temporal_demodulated_halves_device, tray_denoise_temporal_demodulated_guided_device and
tray_denoise_temporal_demodulated_two_pass_device share (include/trayhip.h states the three calls): their numpy statements, typed -- compositions
of _tdemod_ref.demodulated_frames, _temporal2_ref.temporal_halves / temporal_guided / two_pass and _first_hit_ref.scale_of --, their bars, the
loader of the host emulation (tests/emu/emu_td2pass.cpp) with its guarded calls, the GPU tests' calls between guard bytes (torch is imported
there, where a GPU is used), and the parser of the stand-in runtime's log for the stub tests.

`frames` is a list of (even, odd, albedo) RGBW films, frames[0] the centre; `guides` a list of (guide_a, guide_b) pairs in the demodulated domain.

The bar is the project's rule and no new number: 4 x the f32 statement's distance from the f64 one, plus 1e-7, times the largest scale of the
centre's albedo, over the whole image, and the same rule over the centre's valid pixels (_tdemod_ref.bar). The factor is what the multiplication
by s_0 does to the filter's error; the halves are not multiplied by it, so their bar is _temporal2_ref.assert_halves' without the factor."""
import ctypes as C
import functools
import os

import numpy as np

import _emu as E
import _first_hit_ref as FH
import _tdemod_ref as TD
import _temporal2_ref as T2
from _denoise_ref import F32, F64, resolve
from _temporal2_ref import same_bits

DEFAULTS2 = T2.DEFAULTS2


# ---- the statements

def pairs_of(frames):
    return [fr[:2] for fr in frames]


def halves_statement(frames, r=7, rt=3, f=3, k=0.45, F=F64):
    """(fa, fb) as RGBW films in F: _temporal2_ref.temporal_halves of the demodulated frames; not remodulated"""
    return T2.temporal_halves(TD.demodulated_frames(frames, F), r, rt, f, k, F)


def guided_statement(frames, guides, r=5, rt=3, f=1, k=1.0, F=F64):
    """out (h, w, 3) in F: _temporal2_ref.temporal_guided of the demodulated frames under the guides as given, times the centre's scale"""
    d = T2.temporal_guided(TD.demodulated_frames(frames, F), guides, r, rt, f, k, F)
    return (d * FH.scale_of(frames[0][2], F)).astype(F)


def two_pass_statement(frames, r=7, rt=3, f=3, k=0.45, r2=5, rt2=3, f2=1, k2=1.0, F=F64, guides=None):
    """out (h, w, 3) in F: _temporal2_ref.two_pass of the demodulated frames, times the centre's scale (guides: _temporal2_ref.pilots of the
    demodulated frames in F, if the caller has them)"""
    d = T2.two_pass(TD.demodulated_frames(frames, F), r, rt, f, k, r2, rt2, f2, k2, F, guides)
    return (d * FH.scale_of(frames[0][2], F)).astype(F)


def composed(two_pass_call, frames):
    """(h, w, 4): identity (c)'s right-hand side -- numpy-f32 demodulation of every frame, two_pass_call(list of (E', O')) -> (h, w, 4), numpy-f32
    remodulation with the centre's scale, weight 1"""
    return TD.composed(two_pass_call, frames)


def demodulated_pairs(frames):
    """the numpy-f32 quotients (E', O') of every frame: what the undemodulated calls are given in the identities"""
    return TD.demodulated_frames(frames, F32)


def assert_scaled(got_rgbw, statement, frames, sure, what):
    """got (h, w, 4) against statement(F) -> (h, w, 3) under the bar of the module comment; sure: the pixels whose own weight is 1"""
    want, f32 = statement(F64), statement(F32)
    err = np.abs(f32.astype(F64) - want)
    s_max = float(FH.scale_of(frames[0][2], F64).max())
    tol = (4.0 * float(err.max()) + 1e-7) * s_max
    tol_sure = (4.0 * (float(err[sure].max()) if sure.any() else 0.0) + 1e-7) * s_max
    got = np.asarray(got_rgbw)
    assert np.isfinite(got).all() and (got[..., 3] == 1.0).all(), f"{what}: a non-finite word or a weight that is not 1"
    diff = np.abs(got[..., :3].astype(F64) - want)
    over = float(diff[sure].max()) if sure.any() else 0.0
    print(f"{what}: kernels - f64 statement = {diff.max():.3e}, f32 statement - f64 statement = {err.max():.3e}, bar {tol:.3e}; "
          f"over the valid pixels {over:.3e}, bar {tol_sure:.3e}")
    assert diff.max() <= tol, f"{what}: {diff.max():.3e} > {tol:.3e} at {np.unravel_index(np.argmax(diff), diff.shape)}"
    assert over <= tol_sure, f"{what}: valid pixels: {over:.3e} > {tol_sure:.3e}"


def assert_halves(got_fa, got_fb, frames, r, rt, f, k, what):
    """(fa, fb) against halves_statement as _temporal2_ref.assert_halves compares: each half's colours under 4 x (f32 - f64 statement) + 1e-7 over
    the whole image and over the centre's valid pixels; the weights are the f32 statement's; a half without weight is 0"""
    want, f32 = halves_statement(frames, r, rt, f, k, F64), halves_statement(frames, r, rt, f, k, F32)
    valid = TD.valid_of(frames)
    for name, got, w64, w32 in zip("AB", (np.asarray(got_fa), np.asarray(got_fb)), want, f32):
        assert np.isfinite(got).all(), f"{what} {name}: non-finite output"
        assert (got[..., 3] == w32[..., 3]).all(), f"{what} {name}: the weights differ from the f32 statement's"
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
    sure = TD.valid_of(frames) & resolve(*guides[0])[0]
    assert_scaled(got, lambda F: guided_statement(frames, guides, r, rt, f, k, F), frames, sure, what)


@functools.lru_cache(None)
def _random_pilots(w, h, n, seed, r, rt, f, k):
    """_temporal2_ref.pilots of the demodulated random_frames in both types: the second pass's parameters do not enter"""
    frames = TD.random_frames(w, h, n + 1, seed)
    return {F: T2.pilots(TD.demodulated_frames(frames, F), r, rt, f, k, F) for F in (F32, F64)}


def assert_two_pass(got, frames, r, rt, f, k, r2, rt2, f2, k2, what, random_key=None):
    """random_key: (w, h, n, seed) if frames is _tdemod_ref.random_frames(w, h, n + 1, seed)"""
    cached = _random_pilots(*random_key, r, rt, f, k) if random_key is not None else {}
    assert_scaled(got, lambda F: two_pass_statement(frames, r, rt, f, k, r2, rt2, f2, k2, F, cached.get(F)), frames, TD.valid_of(frames), what)


def random_guides(w, h, n, seed):
    """n guide pairs in the demodulated domain that are no film of random_frames(w, h, n, seed): other seeds, other invalid pixels"""
    return T2.random_guides(w, h, n, seed)


# ---- the host emulation

@functools.lru_cache(None)
def td2pass_lib():
    deps = [os.path.join(E.EMU_DIR, x) for x in ("hip_emu.h", "emu_denoise.cpp", "emu_guide.cpp", "emu_temporal2.cpp")]
    deps += [os.path.join(E.HIP_DIR, h) for h in ("td2pass_kernels.h", "tdemod_kernels.h", "t2pass_kernels.h", "guide_kernels.h", "block_compact.h",
                                                  "denoise_kernels.h", "dev_libm.h")]
    deps += E.denoise_plan_deps() + [os.path.join(E.EMU_DIR, "denoise_plan_record.h")]
    h = C.CDLL(E.build("libtrayemu_td2pass.so", "emu_td2pass.cpp", deps))
    P = C.POINTER(C.c_void_p)
    u32, f32, ptr = C.c_uint32, C.c_float, C.c_void_p
    h.emu_td2_halves.restype = C.c_int
    h.emu_td2_halves.argtypes = [u32, u32, ptr, ptr, ptr, u32, P, P, P, u32, u32, u32, f32, ptr, ptr, ptr]
    h.emu_td2_guided.restype = C.c_int
    h.emu_td2_guided.argtypes = [u32, u32, ptr, ptr, ptr, ptr, ptr, u32, P, P, P, P, P, u32, u32, u32, f32, ptr, ptr]
    h.emu_td2_two_pass.restype = C.c_int
    h.emu_td2_two_pass.argtypes = [u32, u32, ptr, ptr, ptr, u32, P, P, P, u32, u32, u32, f32, u32, u32, u32, f32, ptr, ptr]
    for name in ("emu_td2_halves_scratch_bytes", "emu_td2_guided_scratch_bytes", "emu_td2_two_pass_scratch_bytes"):
        getattr(h, name).restype = C.c_uint64
        getattr(h, name).argtypes = [u32, u32]
    h.emu_denoise_plan_layout.restype = u32   # (tests/test_denoise_plan.py)
    h.emu_denoise_plan_layout.argtypes = [u32, u32, u32, ptr, u32, ptr]
    h.emu_denoise_plan_launches.restype = u32
    h.emu_denoise_plan_launches.argtypes = [u32, u32]
    return h


def _flat(frames):
    return [x for fr in frames for x in fr]


def run_halves(emu, frames, r, rt, f, k):
    """the 3 (N + 1) launches of one tray_denoise_temporal_demodulated_halves_device call in the emulation, the outputs and the scratch buffer
    between guard words, the films unchanged afterwards; returns (fa, fb)"""
    frames = T2._contiguous(frames)
    h, w = frames[0][0].shape[:2]
    nb = int(emu.emu_td2_halves_scratch_bytes(w, h))
    assert nb == 128 * w * h
    c, nbs = T2._arrays(frames)
    return tuple(T2._emulated(_flat(frames), nb, 2, lambda outs, scr: emu.emu_td2_halves(w, h, *c, len(frames) - 1, *nbs, r, rt, f, k, *outs, scr)))


def run_guided(emu, frames, guides, r, rt, f, k):
    """the 5 (N + 1) launches of one tray_denoise_temporal_demodulated_guided_device call in the emulation"""
    fr, gd = T2._contiguous(frames), T2._contiguous(guides)
    h, w = fr[0][0].shape[:2]
    nb = int(emu.emu_td2_guided_scratch_bytes(w, h))
    assert nb == 176 * w * h
    c, nbs = T2._arrays(fr)
    g, ngs = T2._arrays(gd)
    return T2._emulated(_flat(fr) + _flat(gd), nb, 1,
                        lambda outs, scr: emu.emu_td2_guided(w, h, *c, *g, len(fr) - 1, *nbs, *ngs, r, rt, f, k, outs[0], scr))[0]


def run_two_pass(emu, frames, r, rt, f, k, r2, rt2, f2, k2):
    """the 9 N + 6 launches of one tray_denoise_temporal_demodulated_two_pass_device call in the emulation"""
    frames = T2._contiguous(frames)
    h, w = frames[0][0].shape[:2]
    nb = int(emu.emu_td2_two_pass_scratch_bytes(w, h))
    assert nb == 256 * w * h
    c, nbs = T2._arrays(frames)
    return T2._emulated(_flat(frames), nb, 1,
                        lambda outs, scr: emu.emu_td2_two_pass(w, h, *c, len(frames) - 1, *nbs, r, rt, f, k, r2, rt2, f2, k2, outs[0], scr))[0]


def composition_of_own_calls(halves_call, guided_call, frames, r, rt, f, k, r2, rt2, f2, k2):
    """identity (d)'s right-hand side from this library's own calls: halves_call(frames) -> (fa, fb) over all frames for the centre and of every
    neighbour alone (N = 0), then guided_call(frames, guides)"""
    guides = [halves_call(frames, r, rt, f, k)] + [halves_call([fr], r, rt, f, k) for fr in frames[1:]]
    return guided_call(frames, guides, r2, rt2, f2, k2)


# ---- on the GPU

def halves_guarded(frames, r, rt, f, k):
    """one tray_denoise_temporal_demodulated_halves_device call between guard bytes (_temporal2_ref._guarded); returns (fa, fb)"""
    def call(lib, d, outs, scr, w, h):
        c, nbs = T2._split(d, len(frames), 3)
        return lib.tray_denoise_temporal_demodulated_halves_device(w, h, *c, len(frames) - 1, *nbs, r, rt, f, k, *outs, scr, None)
    return tuple(T2._guarded(_flat(frames), lambda lib: lib.tray_denoise_temporal_demodulated_halves_scratch_bytes, 128, 2, call))


def guided_guarded(frames, guides, r, rt, f, k):
    """one tray_denoise_temporal_demodulated_guided_device call between guard bytes"""
    def call(lib, d, outs, scr, w, h):
        c, nbs = T2._split(d[:3 * len(frames)], len(frames), 3)
        g, ngs = T2._split(d[3 * len(frames):], len(frames), 2)
        return lib.tray_denoise_temporal_demodulated_guided_device(w, h, *c, *g, len(frames) - 1, *nbs, *ngs, r, rt, f, k, outs[0], scr, None)
    return T2._guarded(_flat(frames) + _flat(guides), lambda lib: lib.tray_denoise_temporal_demodulated_guided_scratch_bytes, 176, 1, call)[0]


def two_pass_guarded(frames, r, rt, f, k, r2, rt2, f2, k2):
    """one tray_denoise_temporal_demodulated_two_pass_device call between guard bytes"""
    def call(lib, d, outs, scr, w, h):
        c, nbs = T2._split(d, len(frames), 3)
        return lib.tray_denoise_temporal_demodulated_two_pass_device(w, h, *c, len(frames) - 1, *nbs, r, rt, f, k, r2, rt2, f2, k2, outs[0], scr, None)
    return T2._guarded(_flat(frames), lambda lib: lib.tray_denoise_temporal_demodulated_two_pass_scratch_bytes, 256, 1, call)[0]


# ---- the stand-in runtime's log (tests/stubs/fakehip.c, tests/_stub.py)

PLAIN = (("k_tdm_prepare", "tdm_prepare"), ("k_dn_prepare", "tdm_variance"), ("k_td2_guided_pass", "td2_guided"), ("k_t2p_halves_pass", "t2p_halves"),
         ("k_t2p_guided_pass", "t2p_guided"), ("k_tdm_pass", "tdm_pass"), ("k_first_hit_tiles", "first_hit"))


def launches(log):
    """every launch of a log written without FAKEHIP_TILE_KERNEL, in order, as (name, template argument, grid, block, stream): _guided_ref.launches'
    names for the lines of libtrayhip_denoise.so and libtrayhip_guide.so ("prepare", "filter", "halves", "guided"); of the plain launch lines
    (libtrayhip_td2pass.so, _t2pass.so, _tdemod.so and _firsthit.so have no branch in the stand-in runtime) PLAIN's name for the kernel symbol, with
    its template argument (-1 where it has none) -- "tdm_variance" is a k_dn_prepare<1> of this library or of libtrayhip_tdemod.so: one of
    libtrayhip_denoise.so's would be a `denoise` line --, "pass" per other launch of 512 threads and "other" per other line"""
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
            name = next((nm for key, nm in PLAIN if key in sym), None)
            arg = -1 if name in (None, "tdm_prepare", "first_hit") else _template_arg(sym)
            out.append((name or ("pass" if int(n["block"]) == 512 else "other"), arg, int(n["grid"]), int(n["block"]), n["stream"]))
    return out
