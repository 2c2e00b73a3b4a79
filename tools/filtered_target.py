"""Does stopping on the error of the DENOISED image pay? tray_render_noise_target_filtered_device at 1920 x 1080 on one GPU, against the raw rule
plus the filter and against a uniform render plus the filter at equal time.

    python tools/filtered_target.py [--scenes cornell_box smallpt] [--thresholds 0.3 0.2 0.15 0.1 0.07 0.05] [--repeats 3] [--out profiles/r10_filtered_target.txt]
    python tools/filtered_target.py --kernels-only     # only part (c)

For each scene (16 ... 1024 samples, filter radius 7, patch 3, k 0.45; RMSE against a 4096-spp render of another seed), per threshold, the three
alternating in one process, each warmed up once and repeated --repeats times, times from device events around the whole sequence (median, and
the spread max - min):
  (a) filtered: one tray_render_noise_target_filtered_device call with out_dev; mean samples per pixel; per round the blocks the filter ran over
      (from the returned n_t: round r filters the blocks that hold a tile with n_t >= min_spp 2^r) and the time of one
      tray_denoise_halves_device call over that list on the final films (a replay: its two preparing launches included);
  (b) raw: tray_render_noise_target_device at the same threshold, then tray_denoise_device;
  (c) uniform: the sample ranges [0, n / 2) and [n / 2, n), then tray_denoise_device, with n chosen so that its time is nearest (a)'s.
Then the kernels: k_dn_filter_halves<3> over the whole frame (tray_denoise_halves_device without a list) against k_dn_filter<3>
(tray_denoise_device) on the same films, alternating, radius 7 and 10; both calls include the same two preparing launches.
Prints every line as it is measured and writes them all to --out."""
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
R, F, K = 7, 3, 0.45
BW, BH = 32, 16
LINES = []


def say(line):
    print(line, flush=True)
    LINES.append(line)


def rgb(img):
    with np.errstate(all="ignore"):
        return np.where(img[..., 3:] > 0, img[..., :3].astype(np.float64) / img[..., 3:].astype(np.float64), 0.0)


def rmse(img, ref):
    return float(np.sqrt(np.mean((rgb(img) - ref) ** 2)))


def ptr(t):
    return C.c_void_p(t.data_ptr())


class Bench:
    def __init__(self, scene, hip):
        import torch
        self.torch, self.scene, self.hip, self.lib = torch, scene, hip, T.lib()
        self.dev = scene.device_scene(0, 0)
        self.spp = hip._select_sampler(self.dev, MAX_SPP)
        new = lambda: torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
        self.even, self.odd, self.out, self.fa, self.fb = new(), new(), new(), new(), new()
        self.scratch = torch.empty(int(self.lib.tray_noise_target_filtered_scratch_bytes(W, H)), dtype=torch.uint8, device="cuda:0")
        self.queue = np.array(T.BlockQueue((W, H), (8, 8)).blocks, np.int64).reshape(-1, 2)
        n = len(self.queue)
        self.smp, self.err = np.zeros(n, np.uint32), np.zeros(n, np.float32)
        self.sp, self.ep = self.smp.ctypes.data_as(C.POINTER(C.c_uint32)), self.err.ctypes.data_as(C.POINTER(C.c_float))

    def timed(self, fn, repeats, warm=1):
        """median and spread (max - min) in ms of fn(), between device events, after `warm` unrecorded runs"""
        torch = self.torch
        times = []
        for i in range(warm + repeats):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            torch.cuda.synchronize()
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            if i >= warm:
                times.append(ev[0].elapsed_time(ev[1]))
        return float(np.median(times)), float(max(times) - min(times))

    def clear(self):
        self.even.zero_(); self.odd.zero_()

    def denoise(self, r=R):
        T.check(self.lib.tray_denoise_device(W, H, ptr(self.even), ptr(self.odd), r, F, K, ptr(self.out), ptr(self.scratch), None))

    def halves(self, r=R, blocks=None):
        T.check(self.lib.tray_denoise_halves_device(W, H, ptr(self.even), ptr(self.odd), r, F, K, None if blocks is None else ptr(blocks),
                                                    0 if blocks is None else len(blocks), ptr(self.fa), ptr(self.fb), ptr(self.scratch), None))

    def filtered(self, thr):
        self.clear()
        T.check(self.lib.tray_render_noise_target_filtered_device(self.dev, 0, 0, MIN_SPP, self.spp, thr, self.hip.seed, ptr(self.even), ptr(self.odd), R, F,
                                                                  K, ptr(self.out), ptr(self.scratch), self.sp, self.ep, None))

    def raw(self, thr):
        self.clear()
        T.check(self.lib.tray_render_noise_target_device(self.dev, 0, 0, MIN_SPP, self.spp, thr, self.hip.seed, ptr(self.even), ptr(self.odd), self.sp,
                                                         self.ep, None))
        self.denoise()

    def uniform(self, n):
        self.clear()
        for film, rng in ((self.even, (0, n // 2)), (self.odd, (n // 2, n))):
            self.hip.render_samples_device(self.scene, 0, (0, 0), MAX_SPP, rng, film.data_ptr())
        self.denoise()

    def result(self, ref):
        return rmse(self.out.cpu().numpy(), ref), float(self.smp.mean())

    def rounds(self):
        """per round of the last filtered call: (samples reached, blocks filtered, ms of a halves call over that list on the final films)"""
        torch = self.torch
        bx = (W + BW - 1) // BW
        out, hi = [], MIN_SPP
        while hi <= int(self.smp.max()):
            t = self.queue if hi == MIN_SPP else self.queue[self.smp >= hi]
            blocks = np.unique((t[:, 1] // (BH // 8)) * bx + t[:, 0] // (BW // 8)).astype(np.uint32)
            bl = torch.from_numpy(blocks.view(np.int32)).cuda()
            ms, _ = self.timed(lambda: self.halves(blocks=bl), 3)
            out.append((hi, len(blocks), ms))
            hi *= 2
        return out


def kernels(b, repeats):
    b.uniform(64)
    for r in (7, 10):
        rows = {"k_dn_filter<3>": [], "k_dn_filter_halves<3>": []}
        for _ in range(3):   # alternating
            rows["k_dn_filter<3>"].append(b.timed(lambda: b.denoise(r), repeats))
            rows["k_dn_filter_halves<3>"].append(b.timed(lambda: b.halves(r), repeats))
        for name, v in rows.items():
            med = [m for m, _ in v]
            say(f"kernels radius {r}: {name} + the two preparing launches, whole frame: {np.median(med):.3f} ms (medians of three alternating series "
                f"{', '.join(f'{m:.3f}' for m in med)}; largest spread within a series {max(s for _, s in v):.3f} ms)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scenes", nargs="+", default=["cornell_box", "smallpt"])
    ap.add_argument("--thresholds", nargs="+", type=float, default=[0.3, 0.2, 0.15, 0.1, 0.07, 0.05])
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10_filtered_target.txt"))
    a = ap.parse_args()
    import torch
    say(f"# tools/filtered_target.py: {W} x {H}, {MIN_SPP} ... {MAX_SPP} spp, filter radius {R} patch {F} k {K}, {a.repeats} repeats after one warm-up; "
        f"{torch.cuda.get_device_name(0)}")
    with tempfile.TemporaryDirectory() as d:
        scenes.write_assets(d)
        for i, name in enumerate(a.scenes):
            p = os.path.join(d, name + ".json")
            with open(p, "w") as f:
                json.dump(getattr(scenes, name)(W, H, MAX_SPP), f)
            scene, *_ = T.Scene.load_file(p)
            b = Bench(scene, T.Hip(0, seed=1))
            if i == 0:
                kernels(b, max(a.repeats, 5))
            if a.kernels_only:
                break
            film = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda:0")
            T.Hip(0, seed=4321).render_device(scene, 0, (0, 0), REF_SPP, film.data_ptr())
            torch.cuda.synchronize()
            ref = rgb(film.cpu().numpy())
            b.hip._select_sampler(b.dev, MAX_SPP)
            per_sample, _ = b.timed(lambda: b.uniform(64), 2)   # ms of a 64-sample uniform render + filter: the slope for choosing n
            flt, _ = b.timed(b.denoise, 3)
            per_sample = (per_sample - flt) / 64.0
            say(f"{name}: uniform render {per_sample:.3f} ms per sample per pixel, tray_denoise_device {flt:.2f} ms")
            for thr in a.thresholds:
                ms_f, sp_f = b.timed(lambda: b.filtered(thr), a.repeats)
                q_f, n_f = b.result(ref)
                rounds = b.rounds()
                ms_r, sp_r = b.timed(lambda: b.raw(thr), a.repeats)
                q_r, n_r = b.result(ref)
                n_u = int(min(MAX_SPP, max(2, 2 * round((ms_f - flt) / per_sample / 2))))
                ms_u, sp_u = b.timed(lambda: b.uniform(n_u), a.repeats)
                q_u, _ = b.result(ref)
                say(f"{name} threshold {thr}: filtered rule {n_f:.1f} spp, {ms_f:.1f} ms (spread {sp_f:.1f}), RMSE {q_f:.4e} | raw rule + filter {n_r:.1f} spp, "
                    f"{ms_r:.1f} ms (spread {sp_r:.1f}), RMSE {q_r:.4e} | uniform {n_u} spp + filter {ms_u:.1f} ms (spread {sp_u:.1f}), RMSE {q_u:.4e} | "
                    f"filtered / uniform: time {ms_f / ms_u:.3f}x, RMSE {q_f / q_u:.3f}x; filtered / raw: time {ms_f / ms_r:.3f}x, RMSE {q_f / q_r:.3f}x")
                say(f"{name} threshold {thr}: rounds (samples reached: blocks filtered of {((W + BW - 1) // BW) * ((H + BH - 1) // BH)}, replayed filter ms): "
                    + ", ".join(f"{hi}: {nb}, {ms:.2f}" for hi, nb, ms in rounds))
            scene.release_device()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
