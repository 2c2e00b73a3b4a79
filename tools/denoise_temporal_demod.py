"""The albedo-demodulated temporal filter (tray_denoise_temporal_demodulated_device) on one GPU: what the albedo films cost beside the temporal call
of the same build, and what they buy on a sequence whose textures change from frame to frame.

    python tools/denoise_temporal_demod.py [--repeats 7] [--spp 16 32 64] [--quality-size 640 360] [--time-only | --quality-only]
    python tools/denoise_temporal_demod.py --filter-only     # the calls of (a) once each: the run to put under rocprofv3 --kernel-trace --stats

(a) time at 1920 x 1080, on textured_box's 64-spp half films and albedo films of three seeds standing in for three frames (the filter's time does
    not depend on the image): HIP events around whole calls, the calls alternating in one process, the median and the spread of --repeats runs
    each after a warm-up (tools/denoise_temporal.py's rule) --
      tray_denoise_temporal_device, N = 0 and N = 2 (radius 7, radius_t 3)     k_dn_prepare<0>, <1>, k_tdn_pass<3> per frame
      tray_denoise_temporal_demodulated_device, N = 0 and N = 2               k_tdm_prepare, k_dn_prepare<1>, k_tdm_pass<3> per frame
    The new call reads 16 bytes more per pixel in each of its N + 1 first preparing launches and in its last pass and writes nothing extra: the
    difference is printed beside the temporal call's own spread and beside those bytes at 2, 3 and 4 TB/s.
(b) quality: textured_box as a three-frame sequence (scene_time 1, shutter 0.5), frame 1 with frames 0 and 2 at --spp samples, rendered by
    Hip.render_sequence_denoised's own calls: RMSE of the centre frame noisy, filtered alone, demodulated alone, temporal, temporal + demodulated,
    and the last with the albedo films of the first 4 samples only (feature_spp = 4), against a 4096-spp render of another seed.
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

W, H, REF_SPP = 1920, 1080, 4096
R, RT, F, K = 7, 3, 3, 0.45


def rgb(img):
    with np.errstate(all="ignore"):
        return np.where(img[..., 3:] > 0, img[..., :3].astype(np.float64) / img[..., 3:].astype(np.float64), 0.0)


def rmse(img, ref):
    return float(np.sqrt(np.mean((rgb(img) - ref) ** 2)))


def albedo_film(hip, scene, frame, w, h, spp, feature_spp):
    """the first-hit albedo film of the samples [0, feature_spp) of a frame on the device (one first-hit launch; normal and depth are dropped)"""
    import torch
    films = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0") for _ in range(3)]
    hip.render_first_hit_device(scene, frame, (0, 0), spp, (0, feature_spp), *[t.data_ptr() for t in films])
    torch.cuda.synchronize()
    return films[0]


def frame_films(hip, scene, frame, w, h, spp):
    """(even, odd, albedo) of a frame on the device: the films of [0, spp / 2) and [spp / 2, spp), the first-hit albedo of [0, spp)"""
    import torch
    halves = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    for film, rng in zip(halves, ((0, spp // 2), (spp // 2, spp))):
        hip.render_samples_device(scene, frame, (0, 0), spp, rng, film.data_ptr())
    torch.cuda.synchronize()
    return halves[0], halves[1], albedo_film(hip, scene, frame, w, h, spp, spp)


class Calls:
    """the two calls on device tensors, each between two HIP events"""

    def __init__(self):
        import torch
        self.torch = torch
        self.scratch = torch.empty(int(T.lib().tray_denoise_temporal_demodulated_scratch_bytes(W, H)), dtype=torch.uint8, device="cuda:0")
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

    def temporal(self, frames, demodulated):
        """frames: (even, odd, albedo) tensors, the centre first"""
        n = len(frames) - 1
        ptrs = [(C.c_void_p * max(n, 1))(*[fr[i].data_ptr() for fr in frames[1:]]) for i in range(3)]
        e, o, a = (C.c_void_p(t.data_ptr()) for t in frames[0])
        tail = (R, RT, F, K, C.c_void_p(self.out.data_ptr()), C.c_void_p(self.scratch.data_ptr()), None)
        if demodulated:
            return self.timed(lambda: T.check(T.lib().tray_denoise_temporal_demodulated_device(W, H, e, o, a, n, *ptrs, *tail)))
        return self.timed(lambda: T.check(T.lib().tray_denoise_temporal_device(W, H, e, o, n, ptrs[0], ptrs[1], *tail)))


def time_part(d, repeats, once):
    calls = Calls()
    scene = T.Scene.load_file(scenes.write_textured_box(os.path.join(d, "time"), width=W, height=H, samples=64))[0]
    frames = [frame_films(T.Hip(0, seed=s), scene, 0, W, H, 64) for s in (1, 2, 3)]
    variants = [("temporal N=0", lambda: calls.temporal(frames[:1], False)), ("temporal demodulated N=0", lambda: calls.temporal(frames[:1], True)),
                ("temporal N=2 rt=3", lambda: calls.temporal(frames, False)), ("temporal demodulated N=2 rt=3", lambda: calls.temporal(frames, True))]
    if once:
        for name, fn in variants:
            print(f"(a) {name}: {fn():.3f} ms (one call)", flush=True)
        return {}
    for _, fn in variants:   # (warm-up: code objects loaded, clocks up)
        fn()
    times = {name: [] for name, _ in variants}
    for _ in range(repeats):   # alternating
        for name, fn in variants:
            times[name].append(fn())
    res = {}
    for name, t in times.items():
        res[name] = {"median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t)), "runs": len(t)}
        print(f"(a) {name}: median {np.median(t):.3f} ms of {len(t)} alternating runs ({min(t):.3f} - {max(t):.3f})", flush=True)
    for n in (0, 2):
        plain, demod = (res[f"temporal {what}N={n}" + (" rt=3" if n else "")] for what in ("", "demodulated "))
        extra = 16.0 * W * H * (n + 2)   # one albedo pixel per prepare of the N + 1 frames and in the last pass
        print(f"(a) N={n}: demodulated - temporal = {demod['median_ms'] - plain['median_ms']:+.3f} ms ({100.0 * (demod['median_ms'] / plain['median_ms'] - 1.0):+.2f} %); "
              f"the temporal call's own spread {plain['max_ms'] - plain['min_ms']:.3f} ms; the {extra / 1e6:.0f} MB more it reads are "
              + ", ".join(f"{extra / (tb * 1e9):.3f} ms at {tb} TB/s" for tb in (2, 3, 4)), flush=True)
    scene.release_device()
    return res


def textured_sequence(d, w, h, spp):
    p = scenes.write_textured_box(d, width=w, height=h, samples=spp, scene_time=1.0, shutter_size=0.5)
    with open(p) as fh:
        desc = json.load(fh)
    desc["film"].update({"frames": 3, "end_frame": 2})
    with open(p, "w") as fh:
        json.dump(desc, fh)
    return T.Scene.load_file(p)[0]


def quality_part(d, spps, size):
    import torch
    w, h = size
    scene = textured_sequence(os.path.join(d, "quality"), w, h, max(spps))
    film = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
    T.Hip(0, seed=4321).render_device(scene, 1, (0, 0), REF_SPP, film.data_ptr())
    torch.cuda.synchronize()
    ref = rgb(film.cpu().numpy())
    print(f"(b) textured_box {w} x {h}, frame 1 of 0 - 2: reference {REF_SPP} spp (another seed)", flush=True)
    hip = T.Hip(0, seed=1)
    res = []
    for spp in spps:
        fr = {g: frame_films(hip, scene, g, w, h, spp) for g in (0, 1, 2)}
        few = {g: albedo_film(hip, scene, g, w, h, spp, 4) for g in (0, 1, 2)}
        order = [fr[1], fr[0], fr[2]]
        pairs = [x[:2] for x in order]
        even, odd, albedo = fr[1]
        images = {"noisy": even + odd, "plain": hip.denoise(even, odd, R, F, K), "demodulated": hip.denoise(even, odd, R, F, K, albedo=albedo),
                  "temporal": hip.denoise_temporal(pairs, 0, R, RT, F, K),
                  "temporal_demodulated": hip.denoise_temporal(pairs, 0, R, RT, F, K, albedos=[x[2] for x in order]),
                  "temporal_demodulated_feature_spp_4": hip.denoise_temporal(pairs, 0, R, RT, F, K, albedos=[few[1], few[0], few[2]])}
        row = {"spp": spp, **{"rmse_" + name: rmse(img.cpu().numpy(), ref) for name, img in images.items()}}
        res.append(row)
        best = min(row["rmse_demodulated"], row["rmse_temporal"])
        print(f"(b) {spp} spp: RMSE " + ", ".join(f"{name} {row['rmse_' + name]:.4e}" for name in images)
              + f": temporal + demodulated = {row['rmse_temporal_demodulated'] / best:.3f} x the better of the two existing calls, "
              f"{row['rmse_temporal_demodulated'] / row['rmse_plain']:.3f} x the plain filter; with feature_spp = 4 "
              f"{row['rmse_temporal_demodulated_feature_spp_4'] / best:.3f} x", flush=True)
    scene.release_device()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--spp", nargs="+", type=int, default=[16, 32, 64])
    ap.add_argument("--quality-size", nargs=2, type=int, default=[640, 360])
    ap.add_argument("--filter-only", action="store_true")
    ap.add_argument("--time-only", action="store_true")
    ap.add_argument("--quality-only", action="store_true")
    a = ap.parse_args()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        if not a.quality_only:
            out["time"] = time_part(d, max(a.repeats, 5), a.filter_only)
        if not (a.filter_only or a.time_only):
            out["quality"] = quality_part(d, a.spp, tuple(a.quality_size))
    print(json.dumps(out, allow_nan=True))


if __name__ == "__main__":
    main()
