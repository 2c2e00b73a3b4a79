"""What ONE GPU does with its share of a frame when the frame is split by SAMPLES over N GPUs (tray_multi_set_partition(TRAY_PARTITION_SAMPLES):
every GPU renders every tile, GPU d the sample indices [d spp / N, (d + 1) spp / N)), measured on a 1-GPU box: each of the N ranges through
tray_render_samples_device against the whole frame on the same GPU, for C4 (the dragon, 2048 spp) and C5 by tiles (the tr15_like stand-in,
frame 64, 512 spp). The counterpart of tools/eighth_rate.py, which measures the tile deal.
    python tools/sample_rate.py [N]          (default N = 8)
efficiency ceiling at N = (time of the whole frame / N) / (time of the slowest range); the RCCL sum-reduce comes on top on real hardware."""
import ctypes
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import tray_rust_amd as T
from tray_rust_amd import multi, scenes

W, H = 1920, 1080
n = int(sys.argv[1]) if len(sys.argv) > 1 else 8
hiprt = ctypes.CDLL("libamdhip64.so")
buf = ctypes.c_void_p()
nbytes = W * H * 4 * 4
assert hiprt.hipMalloc(ctypes.byref(buf), ctypes.c_size_t(nbytes)) == 0
hip = T.Hip(0, seed=1)
for name, spp, frame in (("dragon", 2048, 0), ("tr15_like", 512, 64)):
    d = tempfile.mkdtemp(prefix="sample_rate_")
    if name == "dragon": scenes.write_dragon_assets(d, film=(W, H, spp))
    else: scenes.write_tr15_like_assets(d, film=(W, H, spp))
    scene, rt, _, fi = T.Scene.load_file(os.path.join(d, name + ".json"))

    def run_ms(rng, reps):
        best, samples = 1e30, 0
        for _ in range(reps):
            assert hiprt.hipMemset(buf, 0, ctypes.c_size_t(nbytes)) == 0
            if rng is None: hip.render_device(scene, frame, (0, 0), spp, buf.value)
            else: hip.render_samples_device(scene, frame, (0, 0), spp, rng, buf.value)
            hiprt.hipDeviceSynchronize()
            t = hip.timing(scene)
            best, samples = min(best, t.render_ms), int(t.samples)
        return best, samples
    run_ms(multi.shard_samples(spp, 0, n), 1)   # warm-up: pools, transform table
    whole, s_all = run_ms(None, 2)
    ranges = [multi.shard_samples(spp, k, n) for k in range(n)]
    times, counts = zip(*(run_ms(r, 2) for r in ranges))
    assert sum(counts) == s_all, (sum(counts), s_all)
    label = f"{name} {spp} spp" + (f" frame {frame}" if frame else "")
    print(f"{label}: whole frame {whole:.1f} ms ({s_all / whole / 1e3:.1f} Msamples/s); {n} sample ranges of {spp // n}: "
          f"{' '.join(f'{t:.1f}' for t in times)} ms -> slowest range {whole / n / max(times):.3f} of 1/{n} of the frame "
          f"(sum of the ranges against the whole frame {whole / sum(times):.3f})", flush=True)
