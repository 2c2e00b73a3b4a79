"""The two-pass temporal filter on albedo-demodulated films (tray_denoise_temporal_demodulated_two_pass_device) on one GPU: what the albedo films
cost beside the two-pass temporal call of the same build, and what the three options together buy on a sequence whose textures change from
frame to frame.

    python tools/denoise_temporal_demod_two_pass.py [--repeats 7] [--quality 160 96 32 --quality 640 360 16 ...] [--time-only | --quality-only]
                                                    [--out FILE]

(a) time at 1920 x 1080, N = 2, at the defaults (7, 3, 3, 0.45) and (5, 3, 1, 1.0), on synthetic films of positive weight and synthetic albedo
    films (the filter's time does not depend on the image): HIP events around whole calls, the calls alternating in one process, the median and
    the spread of --repeats runs each after a warm-up --
      tray_denoise_temporal_two_pass_device N = 2 and tray_denoise_temporal_demodulated_two_pass_device N = 2,
      tray_denoise_temporal_device and tray_denoise_temporal_demodulated_device N = 2 beside them.
    The new call reads 16 bytes more per pixel in the first preparing launch of every frame's films -- N + 1 in the first pass, N more when a
    neighbour is resolved again for the second -- and in its last guided pass, and writes nothing extra: the difference is printed beside the
    two-pass temporal call's own spread and beside those bytes at 2, 3 and 4 TB/s.
(b) quality: textured_box as a three-frame sequence (scene_time 1, shutter 0.5), frame 1 with frames 0 and 2, at each --quality W H SPP: RMSE of
    the centre frame noisy and under the four existing calls (plain, temporal, temporal + demodulated, two-pass temporal) and the new one,
    against a 4096-spp render of another seed.
Prints one line per measurement (and appends them to --out) and a JSON summary at the end."""
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
R2, RT2, F2, K2 = 5, 3, 1, 1.0
QUALITY = [(160, 96, 32), (640, 360, 16), (640, 360, 32), (640, 360, 64)]
LINES = []


def say(text):
    print(text, flush=True)
    LINES.append(text)


def rgb(img):
    with np.errstate(all="ignore"):
        return np.where(img[..., 3:] > 0, img[..., :3].astype(np.float64) / img[..., 3:].astype(np.float64), 0.0)


def rmse(img, ref):
    return float(np.sqrt(np.mean((rgb(img) - ref) ** 2)))


def time_part(repeats):
    import torch
    lib = T.lib()
    T.check(lib.tray_init(0))
    gen = torch.Generator(device="cuda:0").manual_seed(5)

    def film(lo=0.0, hi=1.0):
        w = torch.rand((H, W, 1), generator=gen, device="cuda:0") * 7.5 + 0.5
        return torch.cat([(torch.rand((H, W, 3), generator=gen, device="cuda:0") * (hi - lo) + lo) * w, w], -1).contiguous()

    frames = [(film(), film(), film(0.1, 0.9)) for _ in range(3)]   # (even, odd, albedo)
    out = torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0")
    scratch = torch.empty(int(lib.tray_denoise_temporal_demodulated_two_pass_scratch_bytes(W, H)), dtype=torch.uint8, device="cuda:0")
    p = lambda t: C.c_void_p(t.data_ptr())
    arr = lambda ts: (C.c_void_p * max(len(ts), 1))(*[t.data_ptr() for t in ts])
    (e, o, a), (nbe, nbo, nba) = frames[0], [arr([fr[i] for fr in frames[1:]]) for i in range(3)]
    first, second, tail = (R, RT, F, K), (R2, RT2, F2, K2), (p(out), p(scratch), None)

    def timed(launch):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        T.check(launch())
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    variants = [
        ("two-pass temporal N=2", lambda: lib.tray_denoise_temporal_two_pass_device(W, H, p(e), p(o), 2, nbe, nbo, *first, *second, *tail)),
        ("two-pass temporal demodulated N=2", lambda: lib.tray_denoise_temporal_demodulated_two_pass_device(W, H, p(e), p(o), p(a), 2, nbe, nbo, nba, *first,
                                                                                                            *second, *tail)),
        ("temporal N=2", lambda: lib.tray_denoise_temporal_device(W, H, p(e), p(o), 2, nbe, nbo, *first, *tail)),
        ("temporal demodulated N=2", lambda: lib.tray_denoise_temporal_demodulated_device(W, H, p(e), p(o), p(a), 2, nbe, nbo, nba, *first, *tail)),
    ]
    for _, fn in variants:   # (warm-up: code objects loaded, clocks up)
        timed(fn)
    times = {name: [] for name, _ in variants}
    for _ in range(repeats):   # alternating
        for name, fn in variants:
            times[name].append(timed(fn))
    res = {}
    for name, t in times.items():
        res[name] = {"median_ms": float(np.median(t)), "min_ms": float(min(t)), "max_ms": float(max(t)), "runs": len(t)}
        say(f"(a) {name}: median {np.median(t):.3f} ms of {len(t)} alternating runs ({min(t):.3f} - {max(t):.3f})")
    plain, demod = res["two-pass temporal N=2"], res["two-pass temporal demodulated N=2"]
    n = 2
    extra = 16.0 * W * H * (2 * n + 2)   # one albedo pixel per k_tdm_prepare (N + 1 in the first pass, N in the second) and in the last guided pass
    say(f"(a) N={n}: demodulated - two-pass temporal = {demod['median_ms'] - plain['median_ms']:+.3f} ms "
        f"({100.0 * (demod['median_ms'] / plain['median_ms'] - 1.0):+.2f} %); the two-pass temporal call's own spread "
        f"{plain['max_ms'] - plain['min_ms']:.3f} ms; the {extra / 1e6:.0f} MB more it reads are "
        + ", ".join(f"{extra / (tb * 1e9):.3f} ms at {tb} TB/s" for tb in (2, 3, 4)))
    return res


def textured_sequence(d, w, h, spp):
    p = scenes.write_textured_box(d, width=w, height=h, samples=spp, scene_time=1.0, shutter_size=0.5)
    with open(p) as fh:
        desc = json.load(fh)
    desc["film"].update({"frames": 3, "end_frame": 2})
    with open(p, "w") as fh:
        json.dump(desc, fh)
    return T.Scene.load_file(p)[0]


def quality_part(d, cases):
    import torch
    res = []
    for w, h in sorted({c[:2] for c in cases}):
        spps = [c[2] for c in cases if c[:2] == (w, h)]
        scene = textured_sequence(os.path.join(d, f"quality_{w}x{h}"), w, h, max(spps))
        film = torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0")
        T.Hip(0, seed=4321).render_device(scene, 1, (0, 0), REF_SPP, film.data_ptr())
        torch.cuda.synchronize()
        ref = rgb(film.cpu().numpy())
        say(f"(b) textured_box {w} x {h}, frame 1 of 0 - 2: reference {REF_SPP} spp (another seed)")
        hip = T.Hip(0, seed=1)
        for spp in spps:
            fr = {}
            for g in (0, 1, 2):
                films = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0") for _ in range(5)]
                for half, rng in zip(films, ((0, spp // 2), (spp // 2, spp))):
                    hip.render_samples_device(scene, g, (0, 0), spp, rng, half.data_ptr())
                hip.render_first_hit_device(scene, g, (0, 0), spp, (0, spp), *[t.data_ptr() for t in films[2:]])
                torch.cuda.synchronize()
                fr[g] = tuple(films[:3])
            order = [fr[1], fr[0], fr[2]]
            pairs, albedos = [x[:2] for x in order], [x[2] for x in order]
            even, odd, _ = fr[1]
            images = {"noisy": even + odd, "plain": hip.denoise(even, odd, R, F, K), "temporal": hip.denoise_temporal(pairs, 0, R, RT, F, K),
                      "temporal_demodulated": hip.denoise_temporal(pairs, 0, R, RT, F, K, albedos=albedos),
                      "temporal_two_pass": hip.denoise_temporal(pairs, 0, R, RT, F, K, passes=2),
                      "temporal_demodulated_two_pass": hip.denoise_temporal_demodulated(pairs, albedos, 0, R, RT, F, K)}
            row = {"width": w, "height": h, "spp": spp, **{"rmse_" + name: rmse(img.cpu().numpy(), ref) for name, img in images.items()}}
            res.append(row)
            best = min(row["rmse_temporal_demodulated"], row["rmse_temporal_two_pass"])
            say(f"(b) {w} x {h}, {spp} spp: RMSE " + ", ".join(f"{name} {row['rmse_' + name]:.4e}" for name in images)
                + f": all three = {row['rmse_temporal_demodulated_two_pass'] / best:.3f} x the better of the two pairs, "
                f"{row['rmse_temporal_demodulated_two_pass'] / row['rmse_plain']:.3f} x the plain filter")
        scene.release_device()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--quality", nargs=3, type=int, action="append", metavar=("W", "H", "SPP"))
    ap.add_argument("--time-only", action="store_true")
    ap.add_argument("--quality-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        if not a.quality_only:
            out["time"] = time_part(max(a.repeats, 5))
        if not a.time_only:
            out["quality"] = quality_part(d, [tuple(q) for q in a.quality] if a.quality else QUALITY)
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(LINES) + "\n")
    print(json.dumps(out, allow_nan=True))


if __name__ == "__main__":
    main()
