"""TR_LEAN_FOLD_MIS_RAY (csrc/hip/dev_integrator.h: the lean tile kernel's re-timed item, which csrc/hip/kernel_fold.hip turns on) in the host
emulation, with the shipped threshold and with every stage C ray folded, against the base kernel's emulation and the oracle. The fold keeps every
camera sample's radiance and the launch's sample, vertex and ray counts and moves only the step a sample finishes in, so the film is the base's up
to the order of its f32 sums; where nothing can be folded -- a delta light, an LFILT kernel -- it is the base's bit for bit. No GPU needed."""
import functools
import os

import numpy as np
import pytest

import tray_rust_amd as T
import _lean_fold_ref as F
import _lean_tiles_ref as R
import _oracle as O
import _parity


def rgb(img):
    return img[..., :3] / np.maximum(img[..., 3:], 1e-20)


def rmse(a, b):
    return float(np.sqrt(np.mean((rgb(a) - rgb(b)) ** 2)))


@pytest.fixture(scope="module")
def libs(built):
    return F.fold_libs()


@functools.lru_cache(None)
def _references(name, w, h, spp, d):
    """(flat scene, base emulation's film and counts, oracle's film and counts): computed once per case, shared by both thresholds, never written"""
    scene = T.Scene.load_file(F.write_case(name, d, w, h, spp))[0]
    flat = scene.flatten(0)
    base, st_base = R.render_base(flat, spp)
    cpu, st = O.render_tiles(flat, spp, seed=R.SEED)
    base.setflags(write=False); cpu.setflags(write=False)
    return scene, flat, base, st_base, cpu, (int(st.samples), int(st.vertices), int(st.rays))


@pytest.mark.parametrize("k", ["shipped", "always"])
@pytest.mark.parametrize("name,w,h,spp", F.CASES, ids=[c[0] for c in F.CASES])
def test_fold_keeps_counts_and_radiance(name, w, h, spp, k, tmp_path_factory, libs):
    d = str(tmp_path_factory.getbasetemp() / ("fold_" + name))
    os.makedirs(d, exist_ok=True)
    _, flat, base, st_base, cpu, st_cpu = _references(name, w, h, spp, d)
    img, st_fold, folded = F.render_fold(libs[k == "always"], flat, spp)
    diff = float(np.abs(img - base).max())
    print(f"   {name} ({k}): samples, vertices, rays, feat = {st_fold}; folded rays {folded}; max |fold - base| {diff:.3e} of {base.max():.3e}; "
          f"RMSE vs oracle fold {rmse(img, cpu):.3e}, base {rmse(base, cpu):.3e}")
    assert st_base[0] == w * h * spp and st_fold == st_base
    if _parity.mode() == "bit":
        assert st_fold[:3] == st_cpu
    assert diff <= 1e-4 * base.max()                       # (the bar of tests/test_gpu_lean_tiles.py: two schedules of the same samples)
    assert rmse(img, cpu) < _parity.film_bar(2e-6)         # (a wrong or dropped MIS term moves wide_light by per cents)
    if name in ("point_light", "smallpt"):                 # a delta light has no MIS query; smallpt runs an LFILT kernel, which compiles the base's text
        assert folded == 0
        assert np.array_equal(img.view(np.uint32), base.view(np.uint32))
    if name in ("cornell_box", "wide_light") and k == "always":
        assert folded > 0
    if name == "cornell_box" and k == "shipped":
        assert folded > 0
    if name == "wide_light_depth1":                        # (paths of at most two vertices: every folded vertex but a first one is the path's last)
        assert st_fold[1] <= 2 * st_fold[0]
