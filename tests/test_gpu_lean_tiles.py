"""libtrayhip_tiles.so on the GPU: the lean tile kernel (csrc/hip/kernel_tiles.h), which whole-frame Path launches of static scenes run by default,
against the base kernel of libtrayhip.so (TRAYHIP_LEAN_TILES=0) on the scenes of tests/test_lean_tiles_emu.py -- the same samples, vertices and
rays, the same film up to the order of its f32 atomic sums, and both the oracle's image."""
import numpy as np
import pytest

import tray_rust_amd as T
import _lean_tiles_ref as R
import _oracle as O

pytestmark = pytest.mark.gpu
W, H, SPP, SEED = 64, 48, 16, R.SEED


def rgb(img):
    return img[..., :3] / np.maximum(img[..., 3:], 1e-20)


def rmse(a, b):
    return float(np.sqrt(np.mean((rgb(a) - rgb(b)) ** 2)))


def render(scene, rt, fi, monkeypatch, lean):
    """one whole-frame launch with the lean (default) or the base kernel; the switch is read when the device scene is created"""
    if lean:
        monkeypatch.delenv("TRAYHIP_LEAN_TILES", raising=False)
    else:
        monkeypatch.setenv("TRAYHIP_LEAN_TILES", "0")
    scene.release_device()
    rt.clear()
    hip = T.Hip(0, seed=SEED)
    hip.render(scene, rt, T.Config(".", "s", SPP, 1, fi, (0, 0)))
    tim = hip.last_timing
    return rt.get_renderf32().reshape(H, W, 4).copy(), (int(tim.samples), int(tim.vertices), int(tim.rays))


@pytest.mark.parametrize("name", R.CASES)
def test_lean_kernel_renders_what_the_base_kernel_renders(name, tmp_path, monkeypatch):
    scene, rt, _, fi = T.Scene.load_file(R.write_case(name, str(tmp_path), W, H, SPP))
    lean, st_lean = render(scene, rt, fi, monkeypatch, True)
    base, st_base = render(scene, rt, fi, monkeypatch, False)
    scene.release_device()
    cpu, st = O.render_tiles(scene.flatten(0), SPP, seed=SEED)
    print(f"   {name}: lean {st_lean}, base {st_base}, oracle {(st.samples, st.vertices, st.rays)}; max |lean - base| {np.abs(lean - base).max():.3e} of {base.max():.3e}; "
          f"RMSE vs oracle lean {rmse(lean, cpu):.3e}, base {rmse(base, cpu):.3e}")
    assert st_lean == st_base and st_lean[0] == W * H * SPP == st.samples
    assert np.allclose(lean, base, rtol=0, atol=1e-4 * base.max())   # (two schedules of the same samples: tests/test_gpu_parity.py)
    for img, counts in ((lean, st_lean), (base, st_base)):           # (the oracle bars of tests/test_gpu_parity.py: test_image_rmse_c1)
        assert abs(counts[1] - int(st.vertices)) <= (2e-4 if name == "dragon" else 1e-4) * st.vertices   # (the MERL dragon: test_dragon_image_rmse)
        assert np.abs(img[..., 3] - cpu[..., 3]).max() < 1e-3 * cpu[..., 3].max()
        assert rmse(img, cpu) < 1e-4


def test_the_default_runs_the_add_on_kernel_and_the_switch_the_base(tmp_path, monkeypatch, capfd):
    monkeypatch.setenv("TRAYHIP_STATS", "1")
    scene, rt, _, fi = T.Scene.load_file(R.write_case("cornell_box", str(tmp_path), W, H, SPP))
    for lean, want in ((True, "lean (libtrayhip_tiles.so)"), (False, "base (libtrayhip.so)")):
        capfd.readouterr()
        render(scene, rt, fi, monkeypatch, lean)
        lines = [l for l in capfd.readouterr().err.splitlines() if l.startswith("[trayhip] tile launch:")]
        assert lines == [f"[trayhip] tile launch: {want} kernel"], lines
    scene.release_device()
