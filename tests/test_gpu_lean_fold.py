"""TR_LEAN_FOLD_MIS_RAY on the GPU (csrc/hip/dev_integrator.h; libtrayhip_foldmis.so, csrc/hip/kernel_fold.h, is compiled with it): the cases of tests/test_lean_fold_emu.py that
tests/test_gpu_lean_tiles.py's eleven scenes do not hold -- every fold meeting LF_LAST, a tile that drains with folded lanes, one tile at 16 spp --
through the default library against the base kernel of libtrayhip.so (TRAYHIP_LEAN_TILES=0) and the oracle, with the counts and bars of that test."""
import numpy as np
import pytest

import tray_rust_amd as T
import _lean_fold_ref as F
import _lean_tiles_ref as R
import _oracle as O

pytestmark = pytest.mark.gpu
SEED = R.SEED


def rgb(img):
    return img[..., :3] / np.maximum(img[..., 3:], 1e-20)


def rmse(a, b):
    return float(np.sqrt(np.mean((rgb(a) - rgb(b)) ** 2)))


def render(scene, rt, fi, w, h, spp, monkeypatch, lean):
    """one whole-frame launch with the lean (default) or the base kernel; the switch is read when the device scene is created"""
    if lean:
        monkeypatch.delenv("TRAYHIP_LEAN_TILES", raising=False)
    else:
        monkeypatch.setenv("TRAYHIP_LEAN_TILES", "0")
    scene.release_device()
    rt.clear()
    hip = T.Hip(0, seed=SEED)
    hip.render(scene, rt, T.Config(".", "s", spp, 1, fi, (0, 0)))
    tim = hip.last_timing
    return rt.get_renderf32().reshape(h, w, 4).copy(), (int(tim.samples), int(tim.vertices), int(tim.rays))


def test_the_default_runs_the_folding_kernel_and_the_switch_the_tiles_librarys_own(tmp_path, monkeypatch, capfd):
    """a launch without mis_ray_filter goes to libtrayhip_foldmis.so unless TRAYHIP_LEAN_FOLD=0; smallpt's (mis_ray_filter) never does; same counts either way"""
    monkeypatch.setenv("TRAYHIP_STATS", "1")
    fold_line = "[trayhip] lean tile kernel: the folding instantiation (libtrayhip_foldmis.so)"
    w, h, spp = 64, 48, 16
    counts = {}
    for name, switch, want in (("cornell_box", None, [fold_line]), ("cornell_box", "0", []), ("smallpt", None, [])):
        if switch is None:
            monkeypatch.delenv("TRAYHIP_LEAN_FOLD", raising=False)
        else:
            monkeypatch.setenv("TRAYHIP_LEAN_FOLD", switch)
        scene, rt, _, fi = T.Scene.load_file(R.write_case(name, str(tmp_path), w, h, spp))
        capfd.readouterr()
        _, st = render(scene, rt, fi, w, h, spp, monkeypatch, True)
        err = capfd.readouterr().err.splitlines()
        scene.release_device()
        assert [l for l in err if l.startswith("[trayhip] tile launch:")] == ["[trayhip] tile launch: lean (libtrayhip_tiles.so) kernel"], err
        assert [l for l in err if l.startswith("[trayhip] lean tile kernel:")] == want, (name, switch, err)
        counts[(name, switch)] = st
    assert counts[("cornell_box", None)] == counts[("cornell_box", "0")]


@pytest.mark.parametrize("name", list(F.EXTRA))
def test_folding_kernel_renders_what_the_base_kernel_renders(name, tmp_path, monkeypatch):
    w, h, spp = F.EXTRA[name][1:4]
    scene, rt, _, fi = T.Scene.load_file(F.write_case(name, str(tmp_path), w, h, spp))
    lean, st_lean = render(scene, rt, fi, w, h, spp, monkeypatch, True)
    base, st_base = render(scene, rt, fi, w, h, spp, monkeypatch, False)
    scene.release_device()
    cpu, st = O.render_tiles(scene.flatten(0), spp, seed=SEED)
    print(f"   {name}: lean {st_lean}, base {st_base}, oracle {(st.samples, st.vertices, st.rays)}; max |lean - base| {np.abs(lean - base).max():.3e} of {base.max():.3e}; "
          f"RMSE vs oracle lean {rmse(lean, cpu):.3e}, base {rmse(base, cpu):.3e}")
    assert st_lean == st_base and st_lean[0] == w * h * spp == st.samples
    assert np.allclose(lean, base, rtol=0, atol=1e-4 * base.max())   # (two schedules of the same samples: tests/test_gpu_lean_tiles.py)
    for img, counts in ((lean, st_lean), (base, st_base)):           # (the oracle bars of tests/test_gpu_lean_tiles.py)
        assert abs(counts[1] - int(st.vertices)) <= 1e-4 * st.vertices
        assert np.abs(img[..., 3] - cpu[..., 3]).max() < 1e-3 * cpu[..., 3].max()
        assert rmse(img, cpu) < 1e-4
