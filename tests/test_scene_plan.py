"""The per-scene decisions of csrc/hip/scene_plan.h -- the one copy device_api.hip and the host emulation apply -- read through the emulation's
emu_scene_plan: the kernel choices of the fixture scenes, the traversal stack depth on hand-built flat scenes (the smallest trees that pin the
formula: an error there is an out-of-bounds LDS write on the device), and the dynamic-LDS layout."""
import ctypes as C
import os

import pytest

import tray_rust_amd as T
from tray_rust_amd import _lib as L
from tray_rust_amd import scenes
import _emu as E

GEOM_SPHERE, GEOM_MESH = L.GEOM_SPHERE, L.GEOM_MESH


@pytest.fixture(scope="module")
def fixtures(tmp_path_factory, built):
    """name -> (scene, flat scene at frame 0); the scenes keep the flat scenes' memory alive"""
    d = str(tmp_path_factory.mktemp("plan"))
    scenes.write_assets(d, cornell=(64, 48, 4), small=(64, 48, 4))
    paths = {"cornell_box": os.path.join(d, "cornell_box.json"), "smallpt": os.path.join(d, "smallpt.json"),
             "dragon": scenes.write_dragon_assets(os.path.join(d, "dragon"), film=(64, 48, 4), grid=24, extent=1.0)[0],
             "moving_box": scenes.write_moving_box(os.path.join(d, "moving"), width=64, height=48, samples=4),
             "waving_flag": scenes.write_waving_flag(os.path.join(d, "flag"), grid=12, n_keys=4, width=64, height=48, samples=8, frames=8, scene_time=2.0),
             "tr15_like": scenes.write_tr15_like_assets(os.path.join(d, "tr15"), film=(64, 48, 4), detail=0.02)}
    out = {}
    for name, p in paths.items():
        scene = T.Scene.load_file(p if isinstance(p, str) else p[0])[0]
        out[name] = (scene, scene.flatten(0))
    return out


def test_kernel_choices_of_the_fixture_scenes(fixtures):
    plan = {name: E.scene_plan(flat) for name, (_, flat) in fixtures.items()}
    assert [plan[n]["feat"] for n in ("cornell_box", "smallpt", "dragon")] == [0, 4, 1]   # (FEAT_NONE, FEAT_SPEC, FEAT_MERL: tests/test_device_emulation.py)
    assert plan["smallpt"]["light_filter"] == 1 and plan["cornell_box"]["light_filter"] == 0   # specular lobes / a rectangle light and none
    assert all(p["film_rows_ok"] == 1 for p in plan.values())                                # the default filter
    for name in ("cornell_box", "smallpt", "dragon"):
        assert (plan[name]["deforming"], plan[name]["animated"], plan[name]["anim_debug"], plan[name]["n_moving"]) == (0, 0, 0, 0)
    mb = plan["moving_box"]
    assert (mb["deforming"], mb["animated"], mb["anim_debug"]) == (0, 1, 2) and mb["n_moving"] == 4 and mb["xf_movable"] >= mb["n_moving"]
    fl = plan["waving_flag"]                                                                 # the AnimatedMesh scene of tests/test_animated_mesh.py
    assert (fl["deforming"], fl["animated"], fl["anim_debug"], fl["wavefront"]) == (1, 1, 3, 0)
    assert plan["tr15_like"]["wavefront"] == 1 and all(plan[n]["wavefront"] == 0 for n in plan if n != "tr15_like")   # 59 instances > TR_FLAT_MAX


class HandBuilt:
    """A flat scene of spheres and meshes under a BVH<Instance> given as (interior | leaf) nodes; every mesh is a chain tree of a given depth.
    Only what the plan reads (and what the emulation's scene set-up walks) is filled in; boxes and geometry are zero."""

    def __init__(self, top, instance_mesh_depths):
        """top: nodes in the reference's layout -- ("node", index of the right child) with the left child next, or ("leaf", first, count) over the
        instances in order; instance_mesh_depths: per instance None (a sphere) or the depth of its mesh's tree (a mesh of its own)"""
        f = self.flat = L.TrayFlatScene()
        f.abi_version = 0
        n_inst = len(instance_mesh_depths)
        self.instances = (L.TrayInstance * n_inst)()
        depths = [d for d in instance_mesh_depths if d is not None]
        self.meshes = (L.TrayMesh * max(len(depths), 1))()
        n_nodes = sum(2 * d - 1 for d in depths)
        n_tris = sum(depths)
        self.mesh_nodes = (L.TrayBvhNode * max(n_nodes, 1))()
        self.tri_verts = (L.TrayTriVerts * max(n_tris, 1))()
        self.tri_attrs = (L.TrayTriAttrs * max(n_tris, 1))()
        node0 = tri0 = m = 0
        for i, d in enumerate(instance_mesh_depths):
            self.instances[i].geom_type = GEOM_SPHERE if d is None else GEOM_MESH
            self.instances[i].geom_params[0] = 1.0
            for k in (0, 5, 10, 15):
                self.instances[i].mat[k] = self.instances[i].inv[k] = 1.0
            if d is None:
                continue
            self.instances[i].mesh_id = m
            self.meshes[m] = L.TrayMesh(node0, 2 * d - 1, tri0, d)
            for level in range(d - 1):   # interior node 2 * level: a one-triangle leaf to the left, the rest of the chain to the right
                self.mesh_nodes[node0 + 2 * level].offset = 2 * level + 2
                self.mesh_nodes[node0 + 2 * level + 1].offset, self.mesh_nodes[node0 + 2 * level + 1].count = level, 1
            self.mesh_nodes[node0 + 2 * d - 2].offset, self.mesh_nodes[node0 + 2 * d - 2].count = d - 1, 1
            node0 += 2 * d - 1; tri0 += d; m += 1
        self.top = (L.TrayBvhNode * len(top))()
        for k, nd in enumerate(top):
            if nd[0] == "node":
                self.top[k].offset = nd[1]
            else:
                self.top[k].offset, self.top[k].count = nd[1], nd[2]
        self.order = (C.c_uint32 * n_inst)(*range(n_inst))
        self.materials = (L.TrayMaterial * 1)()   # one matte material
        f.n_instances, f.instances = n_inst, self.instances
        f.n_top_nodes, f.top_nodes = len(top), self.top
        f.n_top_order, f.top_order = n_inst, self.order
        f.n_meshes, f.meshes = len(depths), self.meshes
        f.n_mesh_nodes, f.mesh_nodes = n_nodes, self.mesh_nodes
        f.n_tris, f.tri_verts, f.tri_attrs = n_tris, self.tri_verts, self.tri_attrs
        f.n_materials, f.materials = 1, self.materials
        f.max_depth = 4

    def plan(self, **kw):
        return E.scene_plan(C.pointer(self.flat), **kw)


THREE_AND_ONE = [("node", 2), ("leaf", 0, 3), ("leaf", 3, 1)]   # an interior root; the left leaf holds three instances, the right leaf one


def test_stack_depth_of_a_single_leaf_under_a_single_leaf_is_the_floor():
    p = HandBuilt([("leaf", 0, 1)], [1]).plan()
    assert (p["mesh_depth"], p["depth"]) == (1, 4)


def test_stack_depth_counts_the_pending_far_child_and_the_queued_instances():
    """at the left leaf (depth 2) the stack holds 1 pending far child + 3 queued instances, + 1 spare"""
    p = HandBuilt(THREE_AND_ONE, [None] * 4).plan()
    assert (p["mesh_depth"], p["depth"]) == (0, 5)


@pytest.mark.parametrize("d", [1, 2, 3, 7, 40])
def test_stack_depth_with_a_mesh_on_the_first_of_three_instances(d):
    """while the mesh is traversed: 1 far child of the top level + 2 later instances + the exit-mesh sentinel + d - 1 far children inside the mesh"""
    p = HandBuilt(THREE_AND_ONE, [d, None, None, None]).plan()
    assert p["mesh_depth"] == d and p["depth"] == max(d + 1, max(4, 3 + d) + 1)


def expected_layout(flat, p, coop, film_rows):
    """the layout of scene_plan.h from the plan's depth and its constants: (coop_offset, win_offset, stack_bytes)"""
    fs = flat.contents
    words = p["depth"] * p["TR_BLOCK"]
    small = any(fs.meshes[m].tri_count <= p["TR_COOP_MAX_TRIS"] for m in range(fs.n_meshes))
    coop_offset = words if coop and small and fs.n_instances <= p["TR_FLAT_MAX"] else 0
    if coop_offset:
        words += p["TR_BLOCK"] // 64 * p["TR_COOP_WORDS"]
    win_words = 4 * p["WIN_PLANE"]
    return (coop_offset, 0, 4 * max(words, win_words)) if film_rows else (coop_offset, words, 4 * (words + win_words))


def test_lds_layout(fixtures):
    flats = {name: flat for name, (_, flat) in fixtures.items()}
    small_mesh = HandBuilt([("leaf", 0, 1)], [1])                   # a one-triangle mesh: the cooperative test's area lies behind the stacks ...
    many = HandBuilt([("leaf", 0, 17)], [1] + [None] * 16)          # ... unless BVH<Instance> holds more than TR_FLAT_MAX instances
    deep = HandBuilt(THREE_AND_ONE, [40, 2, None, None])            # stacks larger than the film window, with a small mesh
    flats.update(small_mesh=C.pointer(small_mesh.flat), many=C.pointer(many.flat), deep=C.pointer(deep.flat))
    for h in (small_mesh, many, deep):                              # (the default filter's film: the row-binned film is allowed)
        h.flat.film = flats["cornell_box"].contents.film
    seen = set()
    for name, flat in flats.items():
        for coop in (1, 0):
            for film_rows in (1, 0):
                p = E.scene_plan(flat, coop=coop, film_rows=film_rows)
                assert p["film_rows_ok"] == 1
                got = (p["coop_offset"], p["win_offset"], p["stack_bytes"])
                assert got == expected_layout(flat, p, coop, film_rows), (name, coop, film_rows, p)
                if film_rows:   # the window lies over the stacks
                    assert p["win_offset"] == 0 and p["stack_bytes"] >= 4 * p["WIN_PLANE"] * 4
                else:           # ... or behind the stacks and the cooperative area
                    assert p["win_offset"] * 4 + 4 * p["WIN_PLANE"] * 4 == p["stack_bytes"] and p["win_offset"] >= p["depth"] * p["TR_BLOCK"]
                seen.add((bool(p["coop_offset"]), p["depth"] * p["TR_BLOCK"] > 4 * p["WIN_PLANE"]))
    assert (E.scene_plan(flats["small_mesh"])["coop_offset"], E.scene_plan(flats["many"])["coop_offset"]) == (4 * 256, 0)
    assert seen == {(a, b) for a in (False, True) for b in (False, True)}   # with and without the area; stacks smaller and larger than the window
