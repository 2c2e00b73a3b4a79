"""The lean tile kernel's device code (csrc/hip/kernel_tiles.h: kernels.hip under TR_LEAN_TILES, what libtrayhip_tiles.so is compiled from) in the
host emulation against the base kernel's: every item of TR_LEAN_TILES keeps each camera sample's radiance and the launch's sample, vertex and ray
counts, so the two emulated films -- same fibers, same order of the film's f32 sums -- are equal bit for bit. No GPU needed."""
import os

import numpy as np
import pytest

import tray_rust_amd as T
import _lean_tiles_ref as R
import _parity

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
W, H, SPP = 48, 32, 16


def rgb(img):
    return img[..., :3] / np.maximum(img[..., 3:], 1e-20)


@pytest.fixture(scope="module")
def lean(built):
    return R.lean_lib()


@pytest.mark.parametrize("name", R.CASES)
def test_lean_film_and_counters_are_the_base_kernels(name, tmp_path, lean):
    scene = T.Scene.load_file(R.write_case(name, str(tmp_path), W, H, SPP))[0]
    flat = scene.flatten(0)
    base, st_base = R.render_base(flat, SPP)
    img, st_lean = R.render_lean(flat, SPP)
    print(f"   {name}: samples, vertices, rays, feat = {st_lean}")
    assert st_base[0] == W * H * SPP and st_lean == st_base
    assert np.array_equal(img.view(np.uint32), base.view(np.uint32)), int((img.view(np.uint32) != base.view(np.uint32)).sum())
    # (the cases are what their names say: the feature set of the plan, and paths that end at max_depth where the case is about that)
    feat = {"smallpt": 4, "textured_box": 15, "dragon": 1}.get(name, 0)
    assert st_lean[3] == feat
    if name.startswith("depth"):
        assert st_lean[0] < st_lean[1] <= (int(name[5]) + 1) * st_lean[0]   # (max_depth cuts the paths: at most max_depth + 1 vertices each)


@pytest.mark.parametrize("name", ["cornell_box", "smallpt"])
def test_lean_kernel_matches_the_committed_golden(name, tmp_path, lean):
    g = np.load(os.path.join(GOLDEN, f"{name}_48x32_16spp_seed9.npz"))
    scene = T.Scene.load_file(R.write_case(name, str(tmp_path), W, H, SPP))[0]
    img, (samples, vertices, rays, _) = R.render_lean(scene.flatten(0), SPP)
    assert samples == W * H * SPP
    if _parity.mode() == "bit":
        assert (vertices, rays) == (int(g["vertices"]), int(g["rays"]))
    else:
        assert abs(vertices - int(g["vertices"])) <= 2e-3 * int(g["vertices"])
    assert np.abs(img[..., 3] - g["rgbw"][..., 3]).max() < 1e-4 * g["rgbw"][..., 3].max()
    assert float(np.sqrt(np.mean((rgb(img) - rgb(g["rgbw"])) ** 2))) < _parity.film_bar(2e-6)
