"""Two-pass NL-means (tray_denoise_two_pass_device) at 1920 x 1080 on one GPU: what the second pass costs and what it buys.

    python tools/denoise_two_pass.py [--repeats 7] [--spp 16 64 256] [--time-only | --quality-only]
    python tools/denoise_two_pass.py --filter-only     # three calls each of (a): the run to put under rocprofv3 --kernel-trace --stats

(a) time, on the 64-spp half films of cornell_box and smallpt (the filter's time does not depend on the image): HIP events around whole calls,
    the calls alternating, the median and the spread of --repeats runs each after a warm-up --
      tray_denoise_device (7, 3, 0.45)                     k_dn_prepare<0>, <1>, k_dn_filter<3>: the same build's yardstick
      tray_denoise_two_pass_device, second pass (5, 1, 1)  k_dn_prepare<0>, <1>, k_dn_filter_halves<3>, k_dn_prepare<0>, <1>, k_gdn_filter<1>
      ... second pass (7, 1, 1)                            the wider window of the issue's table
    `two passes` minus `tray_denoise_device` is the second pass: two preparing launches and k_gdn_filter<1> (k_dn_filter_halves<3> costs what
    k_dn_filter<3> costs). Under rocprofv3 --kernel-trace --stats the kernels' own times stand side by side.
(b) quality, per scene and --spp: RMSE of the two range films' sum (noisy), of one pass and of two passes at the defaults, against a 4096-spp
    render of another seed.
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
from tray_rust_amd import _lib as L, scenes  # noqa: E402

W, H, REF_SPP = 1920, 1080, 4096
FIRST = (L.TRAY_DENOISE_RADIUS, L.TRAY_DENOISE_PATCH, L.TRAY_DENOISE_K)
SECOND = (L.TRAY_DENOISE_RADIUS2, L.TRAY_DENOISE_PATCH2, L.TRAY_DENOISE_K2)
SCENES = ("cornell_box", "smallpt")


def rgb(img):
    with np.errstate(all="ignore"):
        return np.where(img[..., 3:] > 0, img[..., :3].astype(np.float64) / img[..., 3:].astype(np.float64), 0.0)


def rmse(img, ref):
    return float(np.sqrt(np.mean((rgb(img) - ref) ** 2)))


def halves(hip, scene, spp):
    """the films of [0, spp / 2) and [spp / 2, spp) of frame 0 on the device"""
    import torch
    films = []
    for rng in ((0, spp // 2), (spp // 2, spp)):
        film = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        hip.render_samples_device(scene, 0, (0, 0), spp, rng, film.data_ptr())
        torch.cuda.synchronize()
        films.append(film)
    return tuple(films)


class Calls:
    """the two calls on device tensors, each between two HIP events"""

    def __init__(self):
        import torch
        self.torch = torch
        self.scratch = torch.empty(int(T.lib().tray_denoise_two_pass_scratch_bytes(W, H)), dtype=torch.uint8, device="cuda:0")
        self.out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
        T.check(T.lib().tray_init(0))

    def timed(self, launch):
        torch = self.torch
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        launch()
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    def one(self, pair):
        return self.timed(lambda: T.check(T.lib().tray_denoise_device(W, H, C.c_void_p(pair[0].data_ptr()), C.c_void_p(pair[1].data_ptr()), *FIRST,
                                                                      C.c_void_p(self.out.data_ptr()), C.c_void_p(self.scratch.data_ptr()), None)))

    def two(self, pair, second=SECOND):
        return self.timed(lambda: T.check(T.lib().tray_denoise_two_pass_device(W, H, C.c_void_p(pair[0].data_ptr()), C.c_void_p(pair[1].data_ptr()), *FIRST,
                                                                               *second, C.c_void_p(self.out.data_ptr()),
                                                                               C.c_void_p(self.scratch.data_ptr()), None)))

    def image(self):
        return self.out.cpu().numpy()


def load(d, name, spp):
    p = os.path.join(d, name + ".json")
    with open(p, "w") as f:
        json.dump(getattr(scenes, name)(W, H, spp), f)
    return T.Scene.load_file(p)[0]


def time_part(d, calls, repeats, once):
    res = {}
    for name in SCENES:
        scene = load(d, name, 64)
        pair = halves(T.Hip(0, seed=1), scene, 64)
        variants = [("tray_denoise_device (7, 3, 0.45)", lambda: calls.one(pair)),
                    ("two passes, second (5, 1, 1.0)", lambda: calls.two(pair)),
                    ("two passes, second (7, 1, 1.0)", lambda: calls.two(pair, (7, 1, 1.0)))]
        if once:
            for what, fn in variants[:2]:
                for _ in range(3):
                    print(f"(a) {name}: {what}: {fn():.3f} ms (one call)", flush=True)
            scene.release_device()
            continue
        for _, fn in variants:   # (warm-up: code objects loaded, clocks up)
            fn()
        times = {what: [] for what, _ in variants}
        for _ in range(repeats):   # alternating
            for what, fn in variants:
                times[what].append(fn())
        res[name] = {}
        for what, t in times.items():
            res[name][what] = {"median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t)), "runs": len(t)}
            print(f"(a) {name}: {what}: median {np.median(t):.3f} ms of {len(t)} alternating runs ({min(t):.3f} - {max(t):.3f})", flush=True)
        m = [res[name][what]["median_ms"] for what, _ in variants]
        print(f"(a) {name}: two passes / one pass = {m[1] / m[0]:.3f} (second pass {m[1] - m[0]:.3f} ms); with radius2 = 7: {m[2] / m[0]:.3f} "
              f"({m[2] - m[0]:.3f} ms)", flush=True)
        scene.release_device()
    return res


def quality_part(d, calls, spps):
    import torch
    res = []
    for name in SCENES:
        scene = load(d, name, max(spps))
        film = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        T.Hip(0, seed=4321).render_device(scene, 0, (0, 0), REF_SPP, film.data_ptr())
        torch.cuda.synchronize()
        ref = rgb(film.cpu().numpy())
        scene.release_device()
        hip = T.Hip(0, seed=1)
        for spp in spps:
            pair = halves(hip, scene, spp)
            noisy = rmse((pair[0] + pair[1]).cpu().numpy(), ref)
            calls.one(pair)
            one = rmse(calls.image(), ref)
            calls.two(pair)
            two = rmse(calls.image(), ref)
            calls.two(pair, (7, 1, 1.0))
            wide = rmse(calls.image(), ref)
            res.append({"scene": name, "spp": spp, "rmse_noisy": noisy, "rmse_one_pass": one, "rmse_two_passes": two, "rmse_two_passes_r2_7": wide})
            print(f"(b) {name} {spp} spp: RMSE noisy {noisy:.4e}, one pass {one:.4e}, two passes {two:.4e} ({two / one:.3f} x one pass); "
                  f"with radius2 = 7: {wide:.4e} ({wide / one:.3f} x)", flush=True)
        scene.release_device()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--spp", nargs="+", type=int, default=[16, 64, 256])
    ap.add_argument("--filter-only", action="store_true")
    ap.add_argument("--time-only", action="store_true")
    ap.add_argument("--quality-only", action="store_true")
    a = ap.parse_args()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        scenes.write_assets(d)
        calls = Calls()
        if not a.quality_only:
            out["time"] = time_part(d, calls, max(a.repeats, 1), a.filter_only)
        if not (a.filter_only or a.time_only):
            out["quality"] = quality_part(d, calls, a.spp)
    print(json.dumps(out, allow_nan=True))


if __name__ == "__main__":
    main()
