"""The temporal NL-means filter (tray_denoise_temporal_device) at 1920 x 1080 on one GPU: what a frame's neighbours cost and what they buy.

    python tools/denoise_temporal.py [--repeats 7] [--spp 16 64 256] [--time-only | --quality-only]
    python tools/denoise_temporal.py --filter-only     # the calls of (a) once each: the run to put under rocprofv3 --kernel-trace --stats

(a) time, on cornell_box's 64-spp half films of three seeds standing in for three frames (the filter's time does not depend on the image):
    HIP events around whole calls, the calls alternating, the median and the spread of --repeats runs each after a warm-up --
      tray_denoise_device (radius 7)                          k_dn_prepare<0>, <1>, k_dn_filter<3> of libtrayhip_denoise.so
      tray_denoise_temporal_device, N = 0                     k_dn_prepare<0>, <1>, k_tdn_pass<3> with the centre as the frame
      ... N = 1 at radius_t 3 and 7, N = 2 at radius_t 3      one / two neighbour passes more
    The two preparing launches are the same kernels in every call, so `N = 0` minus `tray_denoise_device` is k_tdn_pass<3> minus k_dn_filter<3>,
    and `N = 1` minus `N = 0` is one neighbour: its two preparing launches and its pass.
(b) quality: moving_box(frames=48), frames 23 - 25 at --spp samples: RMSE of the centre frame noisy, filtered alone (tray_denoise_device) and
    filtered with its two neighbours, against a 4096-spp render of another seed; the render time of a frame's two half films beside the filters'.
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
FRAMES, CENTRE = 48, 24


def rgb(img):
    with np.errstate(all="ignore"):
        return np.where(img[..., 3:] > 0, img[..., :3].astype(np.float64) / img[..., 3:].astype(np.float64), 0.0)


def rmse(img, ref):
    return float(np.sqrt(np.mean((rgb(img) - ref) ** 2)))


def halves(hip, scene, frame, spp):
    """the films of [0, spp / 2) and [spp / 2, spp) of a frame on the device; returns ((even, odd), the sum of their render_ms)"""
    import torch
    films, ms = [], 0.0
    for rng in ((0, spp // 2), (spp // 2, spp)):
        film = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        hip.render_samples_device(scene, frame, (0, 0), spp, rng, film.data_ptr())
        torch.cuda.synchronize()
        ms += hip.timing(scene).render_ms
        films.append(film)
    return tuple(films), ms


class Calls:
    """the two filters on device tensors, each call between two HIP events"""

    def __init__(self):
        import torch
        self.torch = torch
        self.scratch = torch.empty(int(T.lib().tray_denoise_temporal_scratch_bytes(W, H)), dtype=torch.uint8, device="cuda:0")
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

    def spatial(self, pair, radius=R):
        return self.timed(lambda: T.check(T.lib().tray_denoise_device(W, H, C.c_void_p(pair[0].data_ptr()), C.c_void_p(pair[1].data_ptr()), radius, F, K,
                                                                      C.c_void_p(self.out.data_ptr()), C.c_void_p(self.scratch.data_ptr()), None)))

    def temporal(self, centre, neighbours, radius=R, radius_t=RT):
        n = len(neighbours)
        ptrs = [(C.c_void_p * max(n, 1))(*[p[i].data_ptr() for p in neighbours]) for i in range(2)]
        return self.timed(lambda: T.check(T.lib().tray_denoise_temporal_device(
            W, H, C.c_void_p(centre[0].data_ptr()), C.c_void_p(centre[1].data_ptr()), n, ptrs[0], ptrs[1], radius, radius_t, F, K,
            C.c_void_p(self.out.data_ptr()), C.c_void_p(self.scratch.data_ptr()), None)))

    def image(self):
        return self.out.cpu().numpy()


def load(d, name, desc):
    p = os.path.join(d, name + ".json")
    with open(p, "w") as f:
        json.dump(desc, f)
    return T.Scene.load_file(p)[0]


def time_part(d, calls, repeats, once):
    scene = load(d, "cornell_box", scenes.cornell_box(W, H, 64))
    pairs = [halves(T.Hip(0, seed=s), scene, 0, 64)[0] for s in (1, 2, 3)]
    variants = [("tray_denoise_device r=7", lambda: calls.spatial(pairs[0])),
                ("temporal N=0 r=7", lambda: calls.temporal(pairs[0], [])),
                ("temporal N=1 rt=3", lambda: calls.temporal(pairs[0], pairs[1:2])),
                ("temporal N=1 rt=7", lambda: calls.temporal(pairs[0], pairs[1:2], radius_t=7)),
                ("temporal N=2 rt=3", lambda: calls.temporal(pairs[0], pairs[1:]))]
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
    m = lambda name: res[name]["median_ms"]
    print(f"(a) k_tdn_pass<3> (centre as the frame) - k_dn_filter<3> = {m('temporal N=0 r=7') - m('tray_denoise_device r=7'):+.3f} ms "
          f"({100.0 * (m('temporal N=0 r=7') / m('tray_denoise_device r=7') - 1.0):+.1f} % of the call); one neighbour (two preparing launches + pass): "
          f"rt=3 {m('temporal N=1 rt=3') - m('temporal N=0 r=7'):.3f} ms, rt=7 {m('temporal N=1 rt=7') - m('temporal N=0 r=7'):.3f} ms; "
          f"N=2 call / single-frame call = {m('temporal N=2 rt=3') / m('tray_denoise_device r=7'):.3f}", flush=True)
    scene.release_device()
    return res


def quality_part(d, calls, spps):
    scene = load(d, "moving_box", scenes.moving_box(W, H, max(spps), frames=FRAMES))
    ref_film, ref_ms = reference(T.Hip(0, seed=4321), scene)
    ref = rgb(ref_film)
    print(f"(b) moving_box frame {CENTRE}: reference {REF_SPP} spp (another seed) in {ref_ms:.0f} ms", flush=True)
    res = []
    hip = T.Hip(0, seed=1)
    for spp in spps:
        pairs, ms = {}, {}
        for g in (CENTRE - 1, CENTRE, CENTRE + 1):
            pairs[g], ms[g] = halves(hip, scene, g, spp)
        noisy = rmse((pairs[CENTRE][0] + pairs[CENTRE][1]).cpu().numpy(), ref)
        calls.spatial(pairs[CENTRE])
        t_one = calls.spatial(pairs[CENTRE])
        one = rmse(calls.image(), ref)
        calls.temporal(pairs[CENTRE], [pairs[CENTRE - 1], pairs[CENTRE + 1]])
        t_three = calls.temporal(pairs[CENTRE], [pairs[CENTRE - 1], pairs[CENTRE + 1]])
        three = rmse(calls.image(), ref)
        res.append({"spp": spp, "render_ms_per_frame": ms[CENTRE], "rmse_noisy": noisy, "rmse_spatial": one, "spatial_ms": t_one, "rmse_temporal": three,
                    "temporal_ms": t_three})
        print(f"(b) {spp} spp: a frame's two half films {ms[CENTRE]:.1f} ms; RMSE noisy {noisy:.4e}, spatial {one:.4e} ({t_one:.2f} ms), temporal N=2 {three:.4e} "
              f"({t_three:.2f} ms): temporal / spatial = {three / one:.3f}", flush=True)
    scene.release_device()
    return res


def reference(hip, scene):
    """(the 4096-spp film of the centre frame as a numpy array, render_ms)"""
    import torch
    film = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
    hip.render_device(scene, CENTRE, (0, 0), REF_SPP, film.data_ptr())
    torch.cuda.synchronize()
    return film.cpu().numpy(), hip.timing(scene).render_ms


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
            out["time"] = time_part(d, calls, max(a.repeats, 5), a.filter_only)
        if not (a.filter_only or a.time_only):
            out["quality"] = quality_part(d, calls, a.spp)
    print(json.dumps(out, allow_nan=True))


if __name__ == "__main__":
    main()
