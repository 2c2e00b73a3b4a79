"""The emulation libraries of the features that ship as add-on device libraries (tests/emu/emu_sample_ranges.cpp, emu_noise.cpp, emu_denoise.cpp,
emu_guide.cpp): one loader each -- _emu.build plus the ctypes signatures, loaded once -- and the calls more than one test module makes through
them. A new add-on library's emulation gets a loader here."""
import ctypes as C
import functools
import os

import numpy as np

from tray_rust_amd import _lib as L
import _emu as E
from _ranges import SEED, SPP

F32 = np.float32
GUARD = 64   # floats / words / bytes around every buffer the emulated kernels write
SENTINEL = np.uint32(0xDEADBEEF)


def _hip(*headers):
    return [os.path.join(E.EMU_DIR, "hip_emu.h")] + [os.path.join(E.HIP_DIR, h) for h in headers]


@functools.lru_cache(None)
def ranges_lib():
    """the range entry points next to everything emu_kernels.cpp has (emu_sample_ranges.cpp includes it)"""
    h = C.CDLL(E.build("libtrayemu_ranges.so", "emu_sample_ranges.cpp", E.device_deps() + [os.path.join(E.EMU_DIR, "emu_kernels.cpp")]))
    head = [C.POINTER(L.TrayFlatScene), C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32]
    for name, tail in (("tiles", [C.c_int, C.c_int, C.c_void_p]), ("wavefront", [C.c_uint32, C.c_void_p]), ("sampler", [C.c_void_p])):
        fn = getattr(h, f"emu_render_{name}_range")
        fn.restype, fn.argtypes = C.c_int, head + tail
    return h


@functools.lru_cache(None)
def noise_lib():
    h = C.CDLL(E.build("libtrayemu_noise.so", "emu_noise.cpp", _hip("noise_kernels.h", "block_compact.h")))
    h.emu_noise_error.restype = C.c_int
    h.emu_noise_error.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float,
                                  C.c_void_p, C.c_void_p, C.c_void_p]
    h.emu_noise_compact.restype = C.c_int
    h.emu_noise_compact.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    return h


@functools.lru_cache(None)
def denoise_lib():
    h = C.CDLL(E.build("libtrayemu_denoise.so", "emu_denoise.cpp", _hip("denoise_kernels.h", "dev_libm.h") + E.denoise_plan_deps()))
    h.emu_denoise.restype = C.c_int
    h.emu_denoise.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_void_p]
    h.emu_denoise_scratch_bytes.restype = C.c_uint64
    h.emu_denoise_scratch_bytes.argtypes = [C.c_uint32, C.c_uint32]
    return h


@functools.lru_cache(None)
def guide_lib():
    h = C.CDLL(E.build("libtrayemu_guide.so", "emu_guide.cpp", _hip("guide_kernels.h", "block_compact.h", "denoise_kernels.h", "dev_libm.h", "noise_kernels.h",
                                                                    "noise_plan.h")
                       + [os.path.join(E.EMU_DIR, f) for f in ("emu_denoise.cpp", "emu_noise.cpp", "noise_plan_record.h")] + E.denoise_plan_deps()))
    h.emu_guide_halves.restype = C.c_int
    h.emu_guide_halves.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_float, C.c_void_p, C.c_uint32, C.c_void_p,
                                   C.c_void_p, C.c_void_p]
    h.emu_guide_mark.restype = C.c_int
    h.emu_guide_mark.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    h.emu_guide_compact.restype = C.c_int
    h.emu_guide_compact.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    return h


def render_range(h, kind, flat, q, rng, spp=SPP, seed=SEED, **kw):
    """one range launch in the emulation (of _ranges' 16-sample frame); returns (rgbw image, (samples, vertices, rays))"""
    fs = flat.contents
    img = np.zeros((fs.film.height, fs.film.width, 4), np.float32)
    st = np.zeros(4, np.uint64)
    q = np.ascontiguousarray(q, np.uint32)
    if kind == "tiles":
        rc = h.emu_render_tiles_range(flat, q.ctypes.data, len(q), spp, rng[0], rng[1], seed, img.ctypes.data, 2, -1, kw.get("film_rows", -1), st.ctypes.data)
    elif kind == "wavefront":
        rc = h.emu_render_wavefront_range(flat, q.ctypes.data, len(q), spp, rng[0], rng[1], seed, img.ctypes.data, 4, 2, st.ctypes.data)
    else:
        rc = h.emu_render_sampler_range(flat, q.ctypes.data, len(q), spp, rng[0], rng[1], seed, img.ctypes.data, 0, st.ctypes.data)
    assert rc == 0, f"{kind} range {rng}: {rc}"
    return img, tuple(int(v) for v in st[:3])


def noise_error(noise, even, odd, tiles, qidx, n_taken, max_spp, threshold, n_queue):
    """k_noise_error over a list of tiles (qidx: their queue indices, None: the list is the queue); returns (error, active, samples) per queue
    entry, 7s and -1s where the kernel wrote nothing"""
    h, w = even.shape[:2]
    tiles = np.ascontiguousarray(tiles, np.uint32)
    err = np.full(n_queue, -1.0, F32)
    active = np.full(n_queue, 7, np.uint32)
    samples = np.full(n_queue, 7, np.uint32)
    q = None if qidx is None else np.ascontiguousarray(qidx, np.uint32)
    rc = noise.emu_noise_error(even.ctypes.data, odd.ctypes.data, w, h, tiles.ctypes.data, None if q is None else q.ctypes.data, len(tiles), n_taken,
                               max_spp, threshold, err.ctypes.data, active.ctypes.data, samples.ctypes.data)
    assert rc == 0
    return err, active, samples


def denoise(emu, even, odd, r, f, k):
    """the three launches of one tray_denoise_device call in the emulation; the output and the scratch buffer lie between guard words"""
    even, odd = np.ascontiguousarray(even, F32), np.ascontiguousarray(odd, F32)
    h, w = even.shape[:2]
    out = np.full(h * w * 4 + 2 * GUARD, -7.0, F32)
    nb = int(emu.emu_denoise_scratch_bytes(w, h))
    scratch = np.full(nb + 2 * GUARD, 0xA5, np.uint8)
    rc = emu.emu_denoise(even.ctypes.data, odd.ctypes.data, w, h, r, f, k, out[GUARD:].ctypes.data, scratch[GUARD:].ctypes.data)
    assert rc == 0, rc
    assert (out[:GUARD] == -7.0).all() and (out[-GUARD:] == -7.0).all(), "a write outside the output"
    assert (scratch[:GUARD] == 0xA5).all() and (scratch[-GUARD:] == 0xA5).all(), "a write outside the scratch buffer"
    return out[GUARD:-GUARD].reshape(h, w, 4).copy()


def guide_halves(guide, even, odd, r, f, k, blocks=None, into=None):
    """the launches of one tray_denoise_halves_device call in the emulation; fa, fb and the scratch buffer lie between guard words. `into`: the
    (fa, fb) the call writes into (a block list leaves the other pixels alone); default sentinel words. Returns (fa, fb) as (h, w, 4)."""
    even, odd = np.ascontiguousarray(even, F32), np.ascontiguousarray(odd, F32)
    h, w = even.shape[:2]
    outs = []
    for i in range(2):
        buf = np.full(h * w * 4 + 2 * GUARD, SENTINEL, np.uint32)
        if into is not None:
            buf[GUARD:-GUARD] = into[i].reshape(-1).view(np.uint32)
        outs.append(buf)
    scratch = np.full(w * h * 48 + 2 * GUARD, 0xA5, np.uint8)
    bl = None if blocks is None else np.ascontiguousarray(blocks, np.uint32)
    keep = bl if bl is None or len(bl) else np.zeros(1, np.uint32)   # (an empty list is still a non-null pointer)
    rc = guide.emu_guide_halves(even.ctypes.data, odd.ctypes.data, w, h, r, f, k, None if bl is None else keep.ctypes.data, 0 if bl is None else len(bl),
                                outs[0][GUARD:].ctypes.data, outs[1][GUARD:].ctypes.data, scratch[GUARD:].ctypes.data)
    assert rc == 0, rc
    for buf in outs:
        assert (buf[:GUARD] == SENTINEL).all() and (buf[-GUARD:] == SENTINEL).all(), "a write outside fa / fb"
    assert (scratch[:GUARD] == 0xA5).all() and (scratch[-GUARD:] == 0xA5).all(), "a write outside the scratch buffer"
    return tuple(buf[GUARD:-GUARD].view(F32).reshape(h, w, 4).copy() for buf in outs)
