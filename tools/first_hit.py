"""First-hit films (tray_render_first_hit_device) and albedo-demodulated denoising (tray_denoise_demodulated_device) on one GPU: what they cost
and what demodulation buys.

    python tools/first_hit.py [--repeats 7] [--spp 16 64 256] [--time-only | --quality-only]

(a) time at 1920 x 1080, HIP events around whole calls, the median and the spread of --repeats runs after a warm-up, on cornell_box, the dragon
    and the tr15 stand-in: the first-hit call for 64 and for 8 samples of the 64-sample frame beside tray_render_samples_device for the same 64
    samples (one camera ray against a path's roughly ten).
(b) time of tray_denoise_demodulated_device beside tray_denoise_device and the two-pass call on cornell_box's 64-spp half films: the two
    element-wise launches.
(c) quality on textured_box at 160 x 96, per --spp: RMSE of the two range films' sum (noisy), of the plain filter, of the demodulated one with
    the albedo of every sample and of four, against a 4096-spp render of another seed.
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

W, H, REF_SPP, SPP = 1920, 1080, 4096, 64
QW, QH = 160, 96
FIRST = (L.TRAY_DENOISE_RADIUS, L.TRAY_DENOISE_PATCH, L.TRAY_DENOISE_K)
SECOND = (L.TRAY_DENOISE_RADIUS2, L.TRAY_DENOISE_PATCH2, L.TRAY_DENOISE_K2)


def rgb(img):
    with np.errstate(all="ignore"):
        return np.where(img[..., 3:] > 0, img[..., :3].astype(np.float64) / img[..., 3:].astype(np.float64), 0.0)


def rmse(img, ref):
    return float(np.sqrt(np.mean((rgb(img) - ref) ** 2)))


def timed(launch):
    import torch
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    launch()
    ev[1].record()
    torch.cuda.synchronize()
    return ev[0].elapsed_time(ev[1])


def medians(variants, repeats):
    """{what: stats} of alternating runs after one warm-up each"""
    for _, fn in variants:
        fn()
    times = {what: [] for what, _ in variants}
    for _ in range(repeats):
        for what, fn in variants:
            times[what].append(fn())
    return {what: {"median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t)), "runs": len(t)} for what, t in times.items()}


def load_scenes(d):
    out = {}
    scenes.write_assets(d)
    p = os.path.join(d, "cornell.json")
    with open(p, "w") as f:
        json.dump(scenes.cornell_box(W, H, SPP), f)
    out["cornell_box"] = T.Scene.load_file(p)[0]
    out["dragon"] = T.Scene.load_file(scenes.write_dragon_assets(os.path.join(d, "dragon"), film=(W, H, SPP), grid=330)[0])[0]
    out["tr15_like"] = T.Scene.load_file(scenes.write_tr15_like_assets(os.path.join(d, "tr15"), film=(W, H, SPP), detail=0.3)[0])[0]
    return out


def render_part(d, repeats):
    import torch
    res = {}
    hip = T.Hip(0, seed=1)
    films = [torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(4)]
    for name, scene in load_scenes(d).items():
        first = lambda n: timed(lambda: hip.render_first_hit_device(scene, 0, (0, 0), SPP, (0, n), *[f.data_ptr() for f in films[:3]]))
        variants = [(f"tray_render_samples_device, {SPP} samples", lambda: timed(lambda: hip.render_samples_device(scene, 0, (0, 0), SPP, (0, SPP), films[3].data_ptr()))),
                    (f"tray_render_first_hit_device, {SPP} samples", lambda: first(SPP)),
                    ("tray_render_first_hit_device, 8 samples", lambda: first(8))]
        res[name] = medians(variants, repeats)
        m = [res[name][what]["median_ms"] for what, _ in variants]
        for what, _ in variants:
            s = res[name][what]
            print(f"(a) {name}: {what}: median {s['median_ms']:.3f} ms of {s['runs']} runs ({s['min_ms']:.3f} - {s['max_ms']:.3f})", flush=True)
        print(f"(a) {name}: first hit / render = {m[1] / m[0]:.3f} at {SPP} samples, {m[2] / m[0]:.3f} with 8 feature samples", flush=True)
        scene.release_device()
    return res


def filter_part(d, repeats):
    import torch
    p = os.path.join(d, "cornell_f.json")
    with open(p, "w") as f:
        json.dump(scenes.cornell_box(W, H, SPP), f)
    scene = T.Scene.load_file(p)[0]
    hip = T.Hip(0, seed=1)
    even, odd, albedo, normal, depth, out = (torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(6))
    hip.render_samples_device(scene, 0, (0, 0), SPP, (0, SPP // 2), even.data_ptr())
    hip.render_samples_device(scene, 0, (0, 0), SPP, (SPP // 2, SPP), odd.data_ptr())
    hip.render_first_hit_device(scene, 0, (0, 0), SPP, (0, SPP), albedo.data_ptr(), normal.data_ptr(), depth.data_ptr())
    torch.cuda.synchronize()
    lib = T.lib()
    T.check(lib.tray_init(0))
    scratch = torch.empty(int(lib.tray_denoise_demodulated_scratch_bytes(W, H, SECOND[0])), dtype=torch.uint8, device="cuda:0")
    p_ = lambda t: C.c_void_p(t.data_ptr())
    variants = [("tray_denoise_device", lambda: timed(lambda: T.check(lib.tray_denoise_device(W, H, p_(even), p_(odd), *FIRST, p_(out), p_(scratch), None)))),
                ("tray_denoise_demodulated_device, one pass",
                 lambda: timed(lambda: T.check(lib.tray_denoise_demodulated_device(W, H, p_(even), p_(odd), p_(albedo), *FIRST, 0, 0, 1.0, p_(out), p_(scratch), None)))),
                ("tray_denoise_two_pass_device",
                 lambda: timed(lambda: T.check(lib.tray_denoise_two_pass_device(W, H, p_(even), p_(odd), *FIRST, *SECOND, p_(out), p_(scratch), None)))),
                ("tray_denoise_demodulated_device, two passes",
                 lambda: timed(lambda: T.check(lib.tray_denoise_demodulated_device(W, H, p_(even), p_(odd), p_(albedo), *FIRST, *SECOND, p_(out), p_(scratch), None))))]
    res = medians(variants, repeats)
    for what, _ in variants:
        s = res[what]
        print(f"(b) {what}: median {s['median_ms']:.3f} ms of {s['runs']} runs ({s['min_ms']:.3f} - {s['max_ms']:.3f})", flush=True)
    scene.release_device()
    return res


def quality_part(d, spps):
    import torch
    res = []
    scene = T.Scene.load_file(scenes.write_textured_box(os.path.join(d, "tex"), width=QW, height=QH, samples=max(spps)))[0]
    film = torch.zeros((QH, QW, 4), dtype=torch.float32, device="cuda:0")
    T.Hip(0, seed=4321).render_device(scene, 0, (0, 0), REF_SPP, film.data_ptr())
    torch.cuda.synchronize()
    ref = rgb(film.cpu().numpy())
    scene.release_device()
    hip = T.Hip(0, seed=1)
    for spp in spps:
        films = [torch.zeros((QH, QW, 4), dtype=torch.float32, device="cuda:0") for _ in range(8)]
        even, odd, albedo, few = films[:4]
        hip.render_samples_device(scene, 0, (0, 0), spp, (0, spp // 2), even.data_ptr())
        hip.render_samples_device(scene, 0, (0, 0), spp, (spp // 2, spp), odd.data_ptr())
        hip.render_first_hit_device(scene, 0, (0, 0), spp, (0, spp), albedo.data_ptr(), films[4].data_ptr(), films[5].data_ptr())
        hip.render_first_hit_device(scene, 0, (0, 0), spp, (0, 4), few.data_ptr(), films[6].data_ptr(), films[7].data_ptr())
        torch.cuda.synchronize()
        row = {"scene": "textured_box", "spp": spp, "rmse_noisy": rmse((even + odd).cpu().numpy(), ref),
               "rmse_plain": rmse(hip.denoise(even, odd).cpu().numpy(), ref),
               "rmse_demodulated": rmse(hip.denoise(even, odd, albedo=albedo).cpu().numpy(), ref),
               "rmse_demodulated_4_feature_samples": rmse(hip.denoise(even, odd, albedo=few).cpu().numpy(), ref),
               "rmse_two_passes": rmse(hip.denoise(even, odd, passes=2).cpu().numpy(), ref),
               "rmse_two_passes_demodulated": rmse(hip.denoise(even, odd, passes=2, albedo=albedo).cpu().numpy(), ref)}
        res.append(row)
        print(f"(c) textured_box {QW}x{QH} {spp} spp: RMSE noisy {row['rmse_noisy']:.4e}, plain {row['rmse_plain']:.4e}, demodulated "
              f"{row['rmse_demodulated']:.4e} ({row['rmse_demodulated'] / row['rmse_plain']:.3f} x plain), albedo of 4 samples "
              f"{row['rmse_demodulated_4_feature_samples']:.4e} ({row['rmse_demodulated_4_feature_samples'] / row['rmse_plain']:.3f} x); two passes "
              f"{row['rmse_two_passes']:.4e}, demodulated {row['rmse_two_passes_demodulated']:.4e}", flush=True)
    scene.release_device()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--spp", nargs="+", type=int, default=[16, 64, 256])
    ap.add_argument("--time-only", action="store_true")
    ap.add_argument("--quality-only", action="store_true")
    a = ap.parse_args()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        if not a.quality_only:
            out["render"] = render_part(d, max(a.repeats, 1))
            out["filter"] = filter_part(d, max(a.repeats, 1))
        if not a.time_only:
            out["quality"] = quality_part(d, a.spp)
    print(json.dumps(out, allow_nan=True))


if __name__ == "__main__":
    main()
