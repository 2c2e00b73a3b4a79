"""The neighbour bound of the noise-target calls (tray_scene_set_noise_ratio) at 1920 x 1080 on one GPU: what it does to the border pixels whose
weight a neighbouring tile's negative filter lobes cancel (include/trayhip.h, "Border pixels"), and what it costs.

    python tools/noise_bound.py [--out profiles/r20_noise_bound.txt] [--steps cornell_box smallpt suite smoke bench]

Every step is a child process of its own under `timeout`, and the steps are chained: the first that fails ends the run. A scene's step renders
the uniform 1024-spp frame and then, for thresholds 0.05 and 0.2 and max_ratio 0 (no bound), 2, 4 and 8, tray_render_noise_target_device at
16..1024 spp, and records per call: the pixels with weight w <= 0 and those whose rgb / w lies outside the uniform render's range of values,
total samples and render_ms (and both against max_ratio 0 of the same process), the largest n_t ratio between neighbouring tiles, and the RMSE
against the uniform render over all pixels and without those pixels. `suite`, `smoke` and `bench` append the totals of `pytest -m gpu`,
__graft_entry__.smoke() and the plain bench line. Not a test: it asserts nothing about the figures."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, MIN_SPP, MAX_SPP = 1920, 1080, 16, 1024
THRESHOLDS, RATIOS = (0.05, 0.2), (0, 2, 4, 8)
LIMITS = {"suite": 1100, "smoke": 120, "bench": 300}   # seconds per step; a scene's: 600


def scene_step(name):
    sys.path.insert(0, ROOT)
    import torch
    import tray_rust_amd as T
    from tray_rust_amd import scenes
    lib = T.lib()
    with tempfile.TemporaryDirectory() as d:
        scenes.write_assets(d)
        p = os.path.join(d, name + ".json")
        with open(p, "w") as f:
            json.dump(getattr(scenes, name)(W, H, MAX_SPP), f)
        scene, *_ = T.Scene.load_file(p)
    hip = T.Hip(0, seed=1)
    dev = scene.device_scene(0, 0)
    spp = hip._select_sampler(dev, MAX_SPP)
    film = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0")
    hip.render_device(scene, 0, (0, 0), 64, film.data_ptr())   # (warm-up: scene upload, kernels loaded)
    film.zero_()
    hip.render_device(scene, 0, (0, 0), MAX_SPP, film.data_ptr())
    torch.cuda.synchronize()
    t = hip.timing(scene)
    uni = film.cpu().numpy().reshape(H, W, 4).astype(np.float64)
    ref = uni[..., :3] / uni[..., 3:]
    lo, hi = float(ref.min()), float(ref.max())
    print(f"{name} {W}x{H}: uniform {MAX_SPP} spp in {t.render_ms:.1f} ms, {t.samples / 1e9:.3f} G samples, min w {uni[..., 3].min():.2f}, rgb / w in [{lo:.4g}, {hi:.4g}]")
    queue = np.array(T.BlockQueue((W, H), (8, 8)).blocks, np.int64).reshape(-1, 2)
    n = len(queue)
    for thr in THRESHOLDS:
        base = None
        for ratio in RATIOS:
            even = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0")
            odd = torch.zeros_like(even)
            smp, err = np.zeros(n, np.uint32), np.zeros(n, np.float32)
            T.check(lib.tray_scene_set_noise_ratio(dev, ratio))
            T.check(lib.tray_render_noise_target_device(dev, 0, 0, MIN_SPP, spp, thr, hip.seed, C.c_void_p(even.data_ptr()), C.c_void_p(odd.data_ptr()),
                                                        smp.ctypes.data_as(C.POINTER(C.c_uint32)), err.ctypes.data_as(C.POINTER(C.c_float)), None))
            T.check(lib.tray_scene_set_noise_ratio(dev, 0))
            torch.cuda.synchronize()
            t = hip.timing(scene)
            img = (even + odd).cpu().numpy().reshape(H, W, 4).astype(np.float64)
            with np.errstate(all="ignore"):
                x = img[..., :3] / img[..., 3:]
                no_w = img[..., 3] <= 0
                outside = ~no_w & (~np.isfinite(x).all(-1) | (x < lo).any(-1) | (x > hi).any(-1))
                d2 = ((x - ref) ** 2).mean(-1)
            bad = no_w | outside
            rmse_all = float(np.sqrt(d2.mean())) if np.isfinite(d2).all() else float("inf")
            rmse_good = float(np.sqrt(d2[~bad].mean()))
            grid = np.zeros(((H + 7) // 8 + 2, (W + 7) // 8 + 2))
            grid[queue[:, 1] + 1, queue[:, 0] + 1] = smp
            around = np.max([grid[1 + dy:grid.shape[0] - 1 + dy, 1 + dx:grid.shape[1] - 1 + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1)], 0)
            worst = float((around / grid[1:-1, 1:-1]).max())
            if base is None:
                base = (t.samples, t.render_ms)
            print(f"{name} threshold {thr} max_ratio {ratio}: w <= 0 on {int(no_w.sum())} px, rgb / w outside the uniform range on {int(outside.sum())} px, min w "
                  f"{img[..., 3].min():.3f}; {t.samples / 1e9:.3f} G samples ({100.0 * (t.samples / base[0] - 1.0):+.2f} %), {t.render_ms:.1f} ms "
                  f"({100.0 * (t.render_ms / base[1] - 1.0):+.2f} %), {t.launches} launches; largest neighbour ratio {worst:g}; RMSE {rmse_all:.4e}, "
                  f"without those pixels {rmse_good:.4e}", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r20_noise_bound.txt"))
    ap.add_argument("--steps", nargs="+", default=["cornell_box", "smallpt", "suite", "smoke", "bench"])
    ap.add_argument("--scene-step", help="(a child's) render one scene's table")
    a = ap.parse_args()
    if a.scene_step:
        return scene_step(a.scene_step)
    commands = {"suite": [sys.executable, "-m", "pytest", "tests", "-m", "gpu", "-v", "-p", "no:cacheprovider"],   # (-v: a line per test as it ends)
                "smoke": [sys.executable, "-c", "import __graft_entry__ as g; g.smoke()"],
                "bench": [sys.executable, "bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"]}
    with open(a.out, "a") as out:
        for step in a.steps:
            cmd = commands.get(step, [sys.executable, os.path.abspath(__file__), "--scene-step", step])
            child = subprocess.Popen(["timeout", "-k", "10", str(LIMITS.get(step, 600))] + cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
            lines = []
            for line in child.stdout:   # (passed on as it comes: a long step is not silent)
                print(line, end="", flush=True)
                lines.append(line.rstrip("\n"))
            rc = child.wait()
            keep = lines if step not in commands or rc != 0 else [l for l in lines if l.strip()][-1:]
            out.write(f"# {step}: exit status {rc}\n" + "\n".join(keep[-60:]) + "\n")
            out.flush()
            if rc != 0:   # (a failure, a fault or a time limit: nothing more is started)
                return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
