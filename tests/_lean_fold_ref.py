"""The lean tile kernel's re-timed item, TR_LEAN_FOLD_MIS_RAY (csrc/hip/dev_integrator.h), for the CPU and GPU tests: the emulation libraries of
the device code libtrayhip_foldmis.so is compiled from (tests/emu/emu_lean_tiles_fold.cpp, with the shipped threshold and with 65 = every stage C ray
folded), and the cases beyond tests/_lean_tiles_ref.py's that the fold's own branches need."""
import ctypes as C
import functools
import json
import os

import numpy as np

import _emu as E
import _lean_tiles_ref as R

ALWAYS = 65   # TR_LEAN_FOLD_MIN_LANES of the second build: no wave has that many lanes, every stage C ray is folded

# name: (scene, width, height, spp, integrator or None)
EXTRA = {
    "wide_light_depth1": ("wide_light", 48, 32, 16, {"type": "pathtracer", "min_depth": 0, "max_depth": 1}),   # every fold meets LF_LAST
    "wide_light_tile_1spp": ("wide_light", 8, 8, 1, None),     # 64 pairs for 256 lanes: the tile drains with folded lanes
    "wide_light_tile_16spp": ("wide_light", 8, 8, 16, None),
}
CASES = tuple((name, 48, 32, 16) for name in R.CASES) + tuple((name,) + v[1:4] for name, v in EXTRA.items())


def write_case(name, d, w, h, spp):
    if name not in EXTRA:
        return R.write_case(name, d, w, h, spp)
    scene, _, _, _, integrator = EXTRA[name]
    R.scenes.write_assets(d, cornell=(w, h, spp), small=(w, h, spp))
    doc = R._wide_light(w, h, spp)
    if integrator is not None:
        doc["integrator"] = dict(integrator)
    p = os.path.join(d, name + ".json")
    with open(p, "w") as f:
        json.dump(doc, f)
    return p


def _builds():
    deps = E.device_deps() + [os.path.join(E.EMU_DIR, "emu_kernels.cpp")]
    return (("libtrayemu_lean_tiles_fold.so", "emu_lean_tiles_fold.cpp", deps, ()),
            ("libtrayemu_lean_tiles_fold_k65.so", "emu_lean_tiles_fold.cpp", deps, (f"TR_LEAN_FOLD_MIN_LANES={ALWAYS}",)))


@functools.lru_cache(None)
def fold_libs():
    """(the shipped threshold's library, the always-folding one)"""
    libs = []
    for so, src, deps, defines in _builds():
        h = C.CDLL(E.build(so, src, deps, defines=defines))
        h.emu_render_tiles.restype = C.c_int
        h.emu_render_tiles.argtypes = R.lean_lib().emu_render_tiles.argtypes
        h.emu_fold_rays.restype = C.c_ulonglong
        h.emu_fold_min_lanes.restype = C.c_uint
        libs.append(h)
    assert libs[1].emu_fold_min_lanes() == ALWAYS and 1 < libs[0].emu_fold_min_lanes() <= 64
    return tuple(libs)


def render_fold(lib, flat, spp, seed=R.SEED, blocks=2):
    """R.render_lean through one of fold_libs(); returns (rgbw, (samples, vertices, rays, feat), stage C rays folded)"""
    fs = flat.contents
    q = R.tile_queue(fs.film.width, fs.film.height)
    img = np.zeros((fs.film.height, fs.film.width, 4), np.float32)
    stats = np.zeros(4, np.uint64)
    lib.emu_fold_rays()
    rc = lib.emu_render_tiles(flat, q.ctypes.data, len(q), spp, seed, img.ctypes.data, blocks, -1, -1, stats.ctypes.data, 0, 0, 1)
    assert rc == 0, f"emu_render_tiles (fold): {rc}"
    return img, tuple(int(x) for x in stats), int(lib.emu_fold_rays())
