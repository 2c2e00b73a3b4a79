"""The lean tile kernel (libtrayhip_tiles.so, csrc/hip/kernel_tiles.h) for the CPU and GPU tests: the emulation library of its device code
(tests/emu/emu_lean_tiles.cpp = emu_kernels.cpp under TR_LEAN_TILES), and the scenes -- the smallest that reach every branch TR_LEAN_TILES touches."""
import ctypes as C
import functools
import json
import os

import numpy as np

import tray_rust_amd as T
from tray_rust_amd import _lib as L
from tray_rust_amd import scenes
import _emu as E

SEED = 9   # (the seed of tests/golden/*_seed9.npz)


@functools.lru_cache(None)
def lean_lib():
    h = C.CDLL(E.build("libtrayemu_lean_tiles.so", "emu_lean_tiles.cpp", E.device_deps() + [os.path.join(E.EMU_DIR, "emu_kernels.cpp")]))
    h.emu_render_tiles.restype = C.c_int
    h.emu_render_tiles.argtypes = [C.POINTER(L.TrayFlatScene), C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int, C.c_int, C.c_void_p,
                                   C.c_uint32, C.c_uint32, C.c_uint32]
    return h


def tile_queue(width, height):
    return np.array(T.BlockQueue((width, height), (8, 8)).blocks, np.uint32).reshape(-1, 2)


def render_lean(flat, spp, seed=SEED, blocks=2):
    """the emulated lean tile kernel over all tiles, launched as _emu.render_tiles launches the base; returns (rgbw, (samples, vertices, rays, feat))"""
    fs = flat.contents
    q = tile_queue(fs.film.width, fs.film.height)
    img = np.zeros((fs.film.height, fs.film.width, 4), np.float32)
    stats = np.zeros(4, np.uint64)
    rc = lean_lib().emu_render_tiles(flat, q.ctypes.data, len(q), spp, seed, img.ctypes.data, blocks, -1, -1, stats.ctypes.data, 0, 0, 1)
    assert rc == 0, f"emu_render_tiles (lean): {rc}"
    return img, tuple(int(x) for x in stats)


def render_base(flat, spp, seed=SEED, blocks=2):
    fs = flat.contents
    return E.render_tiles(flat, tile_queue(fs.film.width, fs.film.height), spp, seed, blocks=blocks)


def _light(doc):
    return [o for o in doc["objects"] if o.get("type") == "emitter"][0]


def _cornell(w, h, spp, min_depth=None, max_depth=None):
    doc = scenes.cornell_box(w, h, spp)
    if max_depth is not None:
        # (the loader refuses min_depth > max_depth; Russian roulette runs where bounce > min_depth and bounce never passes max_depth, so
        # min_depth = max_depth is the same path tracer as any larger min_depth: no roulette at all)
        doc["integrator"] = {"type": "pathtracer", "min_depth": min(min_depth, max_depth), "max_depth": max_depth}
    return doc


def _wide_light(w, h, spp):
    """cornell_box with the light widened to the whole ceiling: many BSDF samples reach it, the MIS eval pass runs at high lane counts"""
    doc = scenes.cornell_box(w, h, spp)
    _light(doc)["geometry"] = {"type": "rectangle", "width": 30, "height": 40}
    return doc


def _disk_light(w, h, spp):
    doc = scenes.cornell_box(w, h, spp)
    _light(doc)["geometry"] = {"type": "disk", "radius": 3.5, "inner_radius": 0.0}
    return doc


def _point_light(w, h, spp):
    """a delta light: no MIS query at all"""
    doc = scenes.cornell_box(w, h, spp)
    doc["objects"] = [o for o in doc["objects"] if o.get("type") != "emitter"]
    doc["objects"].append({"name": "spark", "type": "emitter", "emitter": "point", "emission": [1, 0.9, 0.8, 400], "transform": [scenes._t(0, 20, 0)]})
    return doc


# depth<max_depth>_min<min_depth>: cornell_box with paths that end at max_depth, with (min 0) and without (min 4) Russian roulette before it
CASES =("cornell_box", "wide_light", "disk_light", "point_light", "smallpt", "textured_box", "dragon",
         "depth1_min0", "depth1_min4", "depth2_min0", "depth2_min4")


def write_case(name, d, w, h, spp):
    """writes the case's scene file and assets under d; returns its path"""
    scenes.write_assets(d, cornell=(w, h, spp), small=(w, h, spp))
    if name == "smallpt":
        return os.path.join(d, "smallpt.json")
    if name == "textured_box":
        return scenes.write_textured_box(d, width=w, height=h, samples=spp)
    if name == "dragon":
        return scenes.write_dragon_assets(d, film=(w, h, spp), grid=16, extent=1.0)[0]
    if name.startswith("depth"):
        doc = _cornell(w, h, spp, min_depth=int(name[-1]), max_depth=int(name[5]))
    else:
        doc = {"cornell_box": scenes.cornell_box, "wide_light": _wide_light, "disk_light": _disk_light, "point_light": _point_light}[name](w, h, spp)
    p = os.path.join(d, name + ".json")
    with open(p, "w") as f:
        json.dump(doc, f)
    return p
