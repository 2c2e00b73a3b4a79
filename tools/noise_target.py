"""Rendering to a noise threshold (tray_render_noise_target_device) at 1920 x 1080 on one GPU, against uniform renders.

    python tools/noise_target.py [--scenes cornell_box smallpt] [--thresholds 0.2 0.05] [--repeats 3]

For each scene:
  (a) overhead at threshold 0: min_spp 16, max_spp 1024 (every tile takes 1024 samples, in 7 rounds of two range launches, the error kernel
      and the compaction) against one tray_render_tiles_device launch at 1024 spp; render_ms of each, alternating, the median of --repeats;
  (b) benefit at each threshold: time, total samples and RMSE against a 4096-spp render, next to a uniform render of the same total sample
      count (the samples [0, n) of the 1024-sample frame for every pixel, n = total / pixels rounded to the nearest integer).
Every image is also checked for DEGENERATE pixels: a total filter weight w <= 0, or a resolved value rgb / w that is not finite or lies more
than ten times beyond the reference's largest. A filter with negative lobes (Mitchell-Netravali) can leave a pixel on the border between tiles
of very different sample counts with almost no weight (include/trayhip.h). The RMSE is reported over all pixels and without the degenerate
ones, with the count and, for each degenerate pixel's tile, the largest ratio of a neighbouring tile's samples to its own.
Prints one line per measurement and a JSON summary at the end."""
import argparse
import ctypes as C
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tray_rust_amd as T  # noqa: E402
from tray_rust_amd import scenes  # noqa: E402

W, H, MIN_SPP, MAX_SPP, REF_SPP = 1920, 1080, 16, 1024, 4096


def resolved(img):
    """rgb / w per pixel in float64 (what RenderTarget's resolve divides), inf / NaN where w is 0"""
    with np.errstate(all="ignore"):
        return img[..., :3].astype(np.float64) / img[..., 3:].astype(np.float64)


def compare(img, ref, smp=None):
    """(degenerate pixels, of them with w <= 0, RMSE over all pixels, RMSE without the degenerate ones, the smallest neighbour-to-own samples ratio
    of a degenerate pixel's tile) -- the ratio only for a noise-target image (smp: its samples per tile in BlockQueue order)"""
    r, x = resolved(ref), resolved(img)
    bound = 10.0 * max(1.0, float(np.abs(r).max()))
    with np.errstate(all="ignore"):
        bad = (img[..., 3] <= 0) | ~np.isfinite(x).all(-1) | (np.abs(x) > bound).any(-1)
        d2 = ((x - r) ** 2).mean(-1)
        every = float(np.sqrt(d2.mean())) if np.isfinite(d2).all() else float("inf")
    good = float(np.sqrt(d2[~bad].mean()))
    ratio = None
    if smp is not None and bad.any():
        n = np.zeros(((H + 7) // 8, (W + 7) // 8), np.int64)
        for (tx, ty), k in zip(T.BlockQueue((W, H), (8, 8)).blocks, smp):
            n[ty, tx] = int(k)
        pad = np.pad(n, 1)
        ratios = [max(pad[ty + dy, tx + dx] for dy in range(3) for dx in range(3)) / n[ty, tx]
                  for ty, tx in {(int(y) // 8, int(x_) // 8) for y, x_ in np.argwhere(bad)}]
        ratio = float(min(ratios))
    return int(bad.sum()), int((img[..., 3] <= 0).sum()), every, good, ratio


def film_of(hip, scene, spp, rng=None):
    import torch
    film = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0")
    if rng is None:
        hip.render_device(scene, 0, (0, 0), spp, film.data_ptr())
    else:
        hip.render_samples_device(scene, 0, (0, 0), spp, rng, film.data_ptr())
    torch.cuda.synchronize()
    t = hip.timing(scene)
    return film.cpu().numpy().reshape(H, W, 4), t.render_ms, int(t.samples)


def noise_target(hip, scene, threshold):
    import torch
    dev = scene.device_scene(0, 0)
    spp = hip._select_sampler(dev, MAX_SPP)
    even = torch.zeros(W * H * 4, dtype=torch.float32, device="cuda:0")
    odd = torch.zeros_like(even)
    torch.cuda.synchronize()
    n = len(T.BlockQueue((W, H), (8, 8)))
    smp, err = np.zeros(n, np.uint32), np.zeros(n, np.float32)
    T.check(T.lib().tray_render_noise_target_device(dev, 0, 0, MIN_SPP, spp, float(threshold), hip.seed, C.c_void_p(even.data_ptr()),
                                                    C.c_void_p(odd.data_ptr()), smp.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                    err.ctypes.data_as(C.POINTER(C.c_float)), None))
    torch.cuda.synchronize()
    t = hip.timing(scene)
    return (even + odd).cpu().numpy().reshape(H, W, 4), t.render_ms, int(t.samples), smp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["cornell_box", "smallpt"])
    ap.add_argument("--thresholds", nargs="+", type=float, default=[0.2, 0.05])
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        scenes.write_assets(d)
        for name in a.scenes:
            p = os.path.join(d, name + ".json")
            with open(p, "w") as f:
                json.dump(getattr(scenes, name)(W, H, MAX_SPP), f)
            scene, *_ = T.Scene.load_file(p)
            hip = T.Hip(0, seed=1)
            film_of(hip, scene, 64)   # (warm-up: scene upload, kernels loaded)
            ref, ref_ms, _ = film_of(hip, scene, REF_SPP)
            print(f"{name}: reference {REF_SPP} spp in {ref_ms:.0f} ms", flush=True)
            res = {"ref_ms": ref_ms}
            plain, noise = [], []
            for _ in range(a.repeats):
                _, ms, _ = film_of(hip, scene, MAX_SPP)
                plain.append(ms)
                _, ms, _, smp = noise_target(hip, scene, 0.0)
                assert (smp == MAX_SPP).all()
                noise.append(ms)
            mp, mn = float(np.median(plain)), float(np.median(noise))
            res["overhead"] = {"tiles_ms": plain, "noise_ms": noise, "ratio": mn / mp}
            print(f"{name} (a) threshold 0, {MIN_SPP}..{MAX_SPP} spp: {mn:.1f} ms against {mp:.1f} ms for tray_render_tiles_device: "
                  f"{100.0 * (mn / mp - 1.0):+.2f} %  (runs {[round(x, 1) for x in noise]} / {[round(x, 1) for x in plain]})", flush=True)
            res["thresholds"] = []
            for thr in a.thresholds:
                img, ms, samples, smp = noise_target(hip, scene, thr)
                n_uni = max(1, min(MAX_SPP, int(round(samples / (W * H)))))
                uni, ms_u, samples_u = film_of(hip, scene, MAX_SPP, (0, n_uni))
                bad, w0, r, r_good, ratio = compare(img, ref, smp)
                bad_u, w0_u, r_u, r_u_good, _ = compare(uni, ref)
                counts = {int(k): int(v) for k, v in zip(*np.unique(smp, return_counts=True))}
                res["thresholds"].append({"threshold": thr, "ms": ms, "samples": samples, "rmse": r, "rmse_without_degenerate": r_good,
                                          "degenerate_pixels": bad, "weight_le_0_pixels": w0, "degenerate_min_neighbour_ratio": ratio,
                                          "tiles_per_spp": counts, "uniform_spp": n_uni, "uniform_ms": ms_u, "uniform_samples": samples_u,
                                          "uniform_rmse": r_u, "uniform_rmse_without_degenerate": r_u_good, "uniform_degenerate_pixels": bad_u})
                print(f"{name} (b) threshold {thr}: {ms:.1f} ms, {samples / 1e9:.3f} G samples ({samples / (W * H):.1f} per pixel), RMSE {r:.4e} "
                      f"({bad} degenerate pixels, {w0} with w <= 0{'' if ratio is None else f', each in a tile with a neighbour of >= {ratio:g}x its samples'}; "
                      f"without them {r_good:.4e}); uniform [0, {n_uni}): {ms_u:.1f} ms, {samples_u / 1e9:.3f} G samples, RMSE {r_u:.4e} "
                      f"({bad_u} degenerate pixels; without them {r_u_good:.4e}); time {ms / ms_u:.3f}x, RMSE without degenerate pixels "
                      f"{r_good / r_u_good:.3f}x the uniform render's; tiles per n_t {counts}", flush=True)
            out[name] = res
            scene.release_device()
    print(json.dumps(out, allow_nan=True))


if __name__ == "__main__":
    main()
