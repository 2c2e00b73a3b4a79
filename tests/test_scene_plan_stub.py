"""The library and the host emulation take a scene's decisions from the one copy in csrc/hip/scene_plan.h: tray_scene_create and one tile-range render
run against the stand-in HIP runtime (tests/stubs/fakehip.c, whose launch line records the dynamic LDS and the kernel's symbol), and the tile kernel's
template arguments and LDS bytes are those of the plan the emulation reports for the same flat scene (tests/_emu.py: scene_plan)."""
import json
import os
import re

import pytest

import tray_rust_amd as T
from tray_rust_amd import scenes
import _emu as E
from _stub import kv, stub   # (stub: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INTEGRATOR_PATH, INTEGRATOR_WHITTED, FEAT_ALL_TEX = 0, 2, 15   # include/trayhip.h; dev_bsdf.h: FEAT_ALL | FEAT_TEX

DRIVER = r'''
import ctypes as C, sys
sys.path.insert(0, %(root)r)
import tray_rust_amd as T
scene = T.Scene.load_file(%(path)r)[0]
hip = T.Hip(device=0, seed=3)
dev = scene.device_scene(0, 0)
film = (C.c_float * (4 * 64 * 48))()
T.check(T.lib().tray_render_tiles_device(dev, 2, 4, 4, 3, C.cast(film, C.c_void_p), None))
print("DONE")
'''


def write(name, d):
    """the scene file of one of the cases, at 64 x 48"""
    if name in ("cornell_box", "smallpt", "whitted"):
        scenes.write_assets(d, cornell=(64, 48, 4), small=(64, 48, 4))
        if name != "whitted":
            return os.path.join(d, name + ".json")
        doc = scenes.smallpt(64, 48, 4)
        doc["integrator"] = {"type": "whitted", "min_depth": 4}
        with open(os.path.join(d, "whitted.json"), "w") as f:
            json.dump(doc, f)
        return os.path.join(d, "whitted.json")
    if name == "moving_box":
        return scenes.write_moving_box(d, width=64, height=48, samples=4)
    return scenes.write_textured_box(d, width=64, height=48, samples=4)


@pytest.mark.parametrize("name", ["cornell_box", "smallpt", "moving_box", "textured_box", "whitted"])
def test_the_library_launches_what_the_plan_says(stub, tmp_path, name, built):
    path = write(name, str(tmp_path))
    scene = T.Scene.load_file(path)[0]
    flat = scene.flatten(0)
    plan = E.scene_plan(flat)
    env = {k: None for k in ("TRAYHIP_MODE", "TRAYHIP_FEAT_ALL", "TRAYHIP_NO_LIGHT_FILTER", "TRAYHIP_DIRECT_FILM", "TRAYHIP_NO_COOP", "FAKEHIP_TILE_KERNEL")}
    out, log = stub(DRIVER % {"root": ROOT, "path": path}, tmp_path, FAKEHIP_DEVICES=1, **env)   # (no override of a decision is inherited)
    assert "DONE" in out.stdout, out.stdout + out.stderr
    launches = [kv(l) for l in log if l.startswith("launch") and "k_path_tiles" in l]
    assert len(launches) == 1, log
    anim, feat, integrator, light_filter = (int(v) for v in re.search(r"k_path_tilesILi(\d+)ELi(\d+)ELi(\d+)ELb([01])EE", launches[0]["kernel"]).groups())
    assert plan["wavefront"] == 0 and plan["deforming"] == 0   # (the tile kernel's scenes; its ANIM is 0 / 1)
    if flat.contents.integrator == INTEGRATOR_WHITTED:         # one instantiation per ANIM (kernel_select.h)
        assert name == "whitted" and (anim, feat, integrator, light_filter) == (plan["animated"], FEAT_ALL_TEX, INTEGRATOR_WHITTED, 0)
    else:
        assert (anim, feat, integrator, light_filter) == (plan["animated"], plan["feat"], INTEGRATOR_PATH, plan["light_filter"])
    assert int(launches[0]["lds"]) == plan["stack_bytes"]
    assert (name != "moving_box" or anim == 1) and (feat == FEAT_ALL_TEX) == (name in ("textured_box", "whitted"))   # (the cases differ)
