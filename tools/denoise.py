"""The dual-buffer NL-means denoiser (tray_denoise_device) at 1920 x 1080 on one GPU: what it costs and what it buys.

    python tools/denoise.py [--scenes cornell_box smallpt] [--spp 64 1024] [--thresholds 0.2 0.05] [--repeats 3]
    python tools/denoise.py --filter-only        # the filter alone on cornell_box's 64-spp films: the run to put under rocprofv3

For each scene:
  (a) time: the two half films of an n-spp frame ([0, n / 2) and [n / 2, n), tray_render_samples_device; render_ms of each) next to the time of
      one tray_denoise_device call on them (HIP events around its three launches, the median of --repeats) for (radius, patch) = (7, 3) and
      (10, 3): the filter's share of a frame;
  (b) quality: RMSE against a 4096-spp render of another seed for: uniform n spp; the same denoised; rendering to a noise threshold (min_spp 16
      of a 1024-sample frame); the same denoised; and a uniform render of the noise-target run's mean sample count, plain and denoised, with
      the times -- the line that says whether adaptive sampling plus the filter beats a uniform render of equal cost.
The per-kernel split (k_dn_prepare / k_dn_filter) comes from `rocprofv3 --kernel-trace --stats -- python tools/denoise.py --filter-only`, the
VALU instruction count from a `--pmc SQ_INSTS_VALU` run of the same command, on its own.
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
CONFIGS = [(7, 3), (10, 3)]
K = 0.45


def rgb(img):
    with np.errstate(all="ignore"):
        return np.where(img[..., 3:] > 0, img[..., :3].astype(np.float64) / img[..., 3:].astype(np.float64), 0.0)


def rmse(img, ref):
    return float(np.sqrt(np.mean((rgb(img) - ref) ** 2)))


def film_of(hip, scene, spp, rng=None):
    """a zeroed device film with the samples rng of the spp-sample frame (None: the whole frame); returns (tensor, render_ms, samples)"""
    import torch
    film = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    if rng is None:
        hip.render_device(scene, 0, (0, 0), spp, film.data_ptr())
    else:
        hip.render_samples_device(scene, 0, (0, 0), spp, rng, film.data_ptr())
    torch.cuda.synchronize()
    t = hip.timing(scene)
    return film, t.render_ms, int(t.samples)


def halves(hip, scene, spp, n):
    """the films of [0, n / 2) and [n / 2, n) of the spp-sample frame; returns (even, odd, the sum of their render_ms)"""
    e, ms_e, _ = film_of(hip, scene, spp, (0, n // 2))
    o, ms_o, _ = film_of(hip, scene, spp, (n // 2, n))
    return e, o, ms_e + ms_o


def noise_target(hip, scene, threshold):
    import torch
    dev = scene.device_scene(0, 0)
    spp = hip._select_sampler(dev, MAX_SPP)
    even = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    odd = torch.zeros_like(even)
    torch.cuda.synchronize()
    n = len(T.BlockQueue((W, H), (8, 8)))
    smp, err = np.zeros(n, np.uint32), np.zeros(n, np.float32)
    T.check(T.lib().tray_render_noise_target_device(dev, 0, 0, MIN_SPP, spp, float(threshold), hip.seed, C.c_void_p(even.data_ptr()),
                                                    C.c_void_p(odd.data_ptr()), smp.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                    err.ctypes.data_as(C.POINTER(C.c_float)), None))
    torch.cuda.synchronize()
    t = hip.timing(scene)
    return even, odd, t.render_ms, int(t.samples)


class Filter:
    """tray_denoise_device on device tensors, timed with HIP events around its three launches"""

    def __init__(self):
        import torch
        self.torch = torch
        self.scratch = torch.empty(int(T.lib().tray_denoise_scratch_bytes(W, H)), dtype=torch.uint8, device="cuda:0")
        self.out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")

    def __call__(self, even, odd, radius, patch, repeats=1):
        torch = self.torch
        times = []
        for _ in range(repeats):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            T.check(T.lib().tray_denoise_device(W, H, C.c_void_p(even.data_ptr()), C.c_void_p(odd.data_ptr()), radius, patch, K,
                                                C.c_void_p(self.out.data_ptr()), C.c_void_p(self.scratch.data_ptr()), None))
            ev[1].record()
            torch.cuda.synchronize()
            times.append(ev[0].elapsed_time(ev[1]))
        return self.out.cpu().numpy(), float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["cornell_box", "smallpt"])
    ap.add_argument("--spp", nargs="+", type=int, default=[64, 1024])
    ap.add_argument("--thresholds", nargs="+", type=float, default=[0.2, 0.05])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--filter-only", action="store_true")
    a = ap.parse_args()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        scenes.write_assets(d)
        for name in (["cornell_box"] if a.filter_only else a.scenes):
            p = os.path.join(d, name + ".json")
            with open(p, "w") as f:
                json.dump(getattr(scenes, name)(W, H, MAX_SPP), f)
            scene, *_ = T.Scene.load_file(p)
            hip = T.Hip(0, seed=1)
            filt = Filter()
            if a.filter_only:
                e, o, _ = halves(hip, scene, 64, 64)
                for r, f in CONFIGS:
                    _, ms = filt(e, o, r, f, a.repeats)
                    print(f"{name} 64 spp: tray_denoise_device(radius {r}, patch {f}) {ms:.2f} ms", flush=True)
                continue
            film_of(hip, scene, 64)   # (warm-up: scene upload, kernels loaded)
            ref_film, ref_ms, _ = film_of(T.Hip(0, seed=4321), scene, REF_SPP)
            ref = rgb(ref_film.cpu().numpy())
            print(f"{name}: reference {REF_SPP} spp (another seed) in {ref_ms:.0f} ms", flush=True)
            res = {"ref_ms": ref_ms, "time": [], "quality": []}
            for n in a.spp:
                e, o, ms = halves(hip, scene, n, n)
                plain = rmse((e + o).cpu().numpy(), ref)
                for r, f in CONFIGS:
                    img, fms = filt(e, o, r, f, a.repeats)
                    q = rmse(img, ref)
                    res["time"].append({"spp": n, "radius": r, "patch": f, "render_ms": ms, "filter_ms": fms, "rmse": plain, "rmse_denoised": q})
                    print(f"{name} (a) {n} spp: two half films {ms:.1f} ms, filter (radius {r}, patch {f}) {fms:.2f} ms = {100.0 * fms / ms:.1f} % of "
                          f"the render; RMSE {plain:.4e} -> {q:.4e} ({q / plain:.3f}x)", flush=True)
            for thr in a.thresholds:
                e, o, ms_nt, samples = noise_target(hip, scene, thr)
                r, f = CONFIGS[0]
                nt_plain = rmse((e + o).cpu().numpy(), ref)
                img, fms = filt(e, o, r, f, a.repeats)
                nt_dn = rmse(img, ref)
                n_uni = max(2, min(MAX_SPP, int(round(samples / (W * H)))))
                e, o, ms_u = halves(hip, scene, MAX_SPP, n_uni)
                u_plain = rmse((e + o).cpu().numpy(), ref)
                img, fms_u = filt(e, o, r, f, a.repeats)
                u_dn = rmse(img, ref)
                res["quality"].append({"threshold": thr, "samples_per_pixel": samples / (W * H), "noise_target_ms": ms_nt, "filter_ms": fms,
                                  "noise_target_rmse": nt_plain, "noise_target_denoised_rmse": nt_dn, "uniform_spp": n_uni, "uniform_ms": ms_u,
                                  "uniform_rmse": u_plain, "uniform_denoised_rmse": u_dn})
                print(f"{name} (b) threshold {thr}: {samples / (W * H):.1f} samples per pixel in {ms_nt:.1f} ms, RMSE {nt_plain:.4e}, denoised "
                      f"(+{fms:.1f} ms) {nt_dn:.4e}; uniform [0, {n_uni}) in two halves {ms_u:.1f} ms, RMSE {u_plain:.4e}, denoised (+{fms_u:.1f} ms) "
                      f"{u_dn:.4e}; noise target + filter against uniform + filter: time {(ms_nt + fms) / (ms_u + fms_u):.3f}x, RMSE {nt_dn / u_dn:.3f}x",
                      flush=True)
            out[name] = res
            scene.release_device()
    print(json.dumps(out, allow_nan=True))


if __name__ == "__main__":
    main()
