"""The two-pass temporal filter (tray_denoise_temporal_two_pass_device) on one GPU: what the second pass over all frames costs beside the temporal
call and the single-frame two-pass call of the same build, and what it buys on a rendered sequence.

    python tools/denoise_temporal_two_pass.py [--repeats 9] [--spp 16 32 64] [--quality-size 640 360] [--time-only | --quality-only] [--out FILE]

(a) time at 1920 x 1080, N = 2, at the defaults (7, 3, 3, 0.45) and (5, 3, 1, 1.0), on synthetic films of positive weight (the filter's time
    does not depend on the image): HIP events around whole calls, the calls alternating in one process, the median and the spread of
    --repeats runs each after a warm-up --
      tray_denoise_temporal_device N = 2, tray_denoise_two_pass_device, tray_denoise_temporal_two_pass_device N = 2,
      and the pieces Hip.render_sequence_denoised(passes=2) makes per frame: tray_denoise_halves_device (a frame's own halves, once per frame),
      tray_denoise_temporal_halves_device N = 2 and tray_denoise_temporal_guided_device N = 2 (also at (7, 3, 3), beside the temporal call's pass).
(b) quality: textured_box as a three-frame sequence (scene_time 1, shutter 0.5), frame 1 with frames 0 and 2 at --spp samples: RMSE of the centre
    frame noisy, plain, two passes of the frame alone, temporal and two-pass temporal against a 4096-spp render of another seed.
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

    def film():
        w = torch.rand((H, W, 1), generator=gen, device="cuda:0") * 7.5 + 0.5
        return torch.cat([torch.rand((H, W, 3), generator=gen, device="cuda:0") * w, w], -1).contiguous()

    frames = [(film(), film()) for _ in range(3)]
    guides = [(film(), film()) for _ in range(3)]
    outs = [torch.empty((H, W, 4), dtype=torch.float32, device="cuda:0") for _ in range(2)]
    scratch = torch.empty(int(lib.tray_denoise_temporal_two_pass_scratch_bytes(W, H)), dtype=torch.uint8, device="cuda:0")
    p = lambda t: C.c_void_p(t.data_ptr())
    arr = lambda ts: (C.c_void_p * max(len(ts), 1))(*[t.data_ptr() for t in ts])
    (e, o), nbe, nbo = frames[0], arr([fr[0] for fr in frames[1:]]), arr([fr[1] for fr in frames[1:]])
    (ga, gb), nga, ngb = guides[0], arr([g[0] for g in guides[1:]]), arr([g[1] for g in guides[1:]])
    out, s = p(outs[0]), p(scratch)

    def timed(launch):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        torch.cuda.synchronize()
        ev[0].record()
        T.check(launch())
        ev[1].record()
        torch.cuda.synchronize()
        return ev[0].elapsed_time(ev[1])

    variants = [
        ("temporal N=2", lambda: lib.tray_denoise_temporal_device(W, H, p(e), p(o), 2, nbe, nbo, R, RT, F, K, out, s, None)),
        ("two-pass, one frame", lambda: lib.tray_denoise_two_pass_device(W, H, p(e), p(o), R, F, K, R2, F2, K2, out, s, None)),
        ("two-pass temporal N=2", lambda: lib.tray_denoise_temporal_two_pass_device(W, H, p(e), p(o), 2, nbe, nbo, R, RT, F, K, R2, RT2, F2, K2, out, s, None)),
        ("halves, one frame", lambda: lib.tray_denoise_halves_device(W, H, p(e), p(o), R, F, K, None, 0, out, p(outs[1]), s, None)),
        ("temporal halves N=2", lambda: lib.tray_denoise_temporal_halves_device(W, H, p(e), p(o), 2, nbe, nbo, R, RT, F, K, out, p(outs[1]), s, None)),
        ("temporal guided N=2 (5, 3, 1)", lambda: lib.tray_denoise_temporal_guided_device(W, H, p(e), p(o), p(ga), p(gb), 2, nbe, nbo, nga, ngb, R2, RT2, F2, K2, out, s, None)),
        ("temporal guided N=2 (7, 3, 3)", lambda: lib.tray_denoise_temporal_guided_device(W, H, p(e), p(o), p(ga), p(gb), 2, nbe, nbo, nga, ngb, R, RT, F, K, out, s, None)),
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
    m = lambda name: res[name]["median_ms"]
    say(f"(a) two-pass temporal / temporal = {m('two-pass temporal N=2') / m('temporal N=2'):.3f}, / two-pass of one frame = "
        f"{m('two-pass temporal N=2') / m('two-pass, one frame'):.3f}")
    per_frame = m("halves, one frame") + m("temporal halves N=2") + m("temporal guided N=2 (5, 3, 1)")
    say(f"(a) per frame inside render_sequence_denoised(passes=2, reach=1): the frame's own halves once + temporal halves + temporal guided = "
        f"{per_frame:.3f} ms, {per_frame / m('temporal N=2'):.3f} x the temporal call, {per_frame / m('two-pass temporal N=2'):.3f} x the stand-alone two-pass call")
    say(f"(a) guided passes beside the temporal call's passes, N = 2: at (5, 3, 1) {m('temporal guided N=2 (5, 3, 1)') / m('temporal N=2'):.3f} x, "
        f"at (7, 3, 3) {m('temporal guided N=2 (7, 3, 3)') / m('temporal N=2'):.3f} x (the guided call makes two more preparing launches per frame "
        f"and loads the values' two records per offset from global memory)")
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
    say(f"(b) textured_box {w} x {h}, frame 1 of 0 - 2: reference {REF_SPP} spp (another seed)")
    hip = T.Hip(0, seed=1)
    res = []
    for spp in spps:
        fr = {}
        for g in (0, 1, 2):
            halves = [torch.zeros((h, w, 4), dtype=torch.float32, device="cuda:0") for _ in range(2)]
            for half, rng in zip(halves, ((0, spp // 2), (spp // 2, spp))):
                hip.render_samples_device(scene, g, (0, 0), spp, rng, half.data_ptr())
            torch.cuda.synchronize()
            fr[g] = tuple(halves)
        pairs = [fr[1], fr[0], fr[2]]
        even, odd = fr[1]
        images = {"noisy": even + odd, "plain": hip.denoise(even, odd, R, F, K), "two_pass": hip.denoise(even, odd, R, F, K, passes=2),
                  "temporal": hip.denoise_temporal(pairs, 0, R, RT, F, K), "temporal_two_pass": hip.denoise_temporal(pairs, 0, R, RT, F, K, passes=2)}
        row = {"spp": spp, **{"rmse_" + name: rmse(img.cpu().numpy(), ref) for name, img in images.items()}}
        res.append(row)
        say(f"(b) {spp} spp: RMSE " + ", ".join(f"{name} {row['rmse_' + name]:.4e}" for name in images)
            + f": two-pass temporal = {row['rmse_temporal_two_pass'] / row['rmse_temporal']:.3f} x the temporal call, "
            f"{row['rmse_temporal_two_pass'] / row['rmse_two_pass']:.3f} x two passes of the frame alone, {row['rmse_temporal_two_pass'] / row['rmse_plain']:.3f} x the plain filter")
    scene.release_device()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--spp", nargs="+", type=int, default=[16, 32, 64])
    ap.add_argument("--quality-size", nargs=2, type=int, default=[640, 360])
    ap.add_argument("--time-only", action="store_true")
    ap.add_argument("--quality-only", action="store_true")
    ap.add_argument("--out")
    a = ap.parse_args()
    out = {}
    with tempfile.TemporaryDirectory() as d:
        if not a.quality_only:
            out["time"] = time_part(max(a.repeats, 5))
        if not a.time_only:
            out["quality"] = quality_part(d, a.spp, tuple(a.quality_size))
    if a.out:
        with open(a.out, "a") as fh:
            fh.write("\n".join(LINES) + "\n")
    print(json.dumps(out, allow_nan=True))


if __name__ == "__main__":
    main()
