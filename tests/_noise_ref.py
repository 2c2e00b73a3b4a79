"""What the tests of the noise target share (include/trayhip.h: tray_render_noise_target_device and, built on it, the filtered rule): the numpy
statement of a tile's error and the ulp bar it is held to, and the helpers of the GPU tests -- scenes, device films, the oracle's film of each
tile's prefix. Nothing here builds or loads an emulation library; torch is imported where a GPU is used."""
import json
import os

import numpy as np

import tray_rust_amd as T
from tray_rust_amd import scenes
import _oracle as O

F32 = np.float32


def numpy_tile_error(even, odd, tile):
    """include/trayhip.h's error of one tile, in float32 and in the header's order of operations"""
    tx, ty = int(tile[0]), int(tile[1])
    E_ = even[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8].reshape(-1, 4)   # (the slice keeps the pixels inside the image)
    O_ = odd[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8].reshape(-1, 4)
    with np.errstate(all="ignore"):
        e, o = E_[:, :3] / E_[:, 3:], O_[:, :3] / O_[:, 3:]
        d = ((np.abs(e[:, 0] - o[:, 0]) + np.abs(e[:, 1] - o[:, 1])) + np.abs(e[:, 2] - o[:, 2])) * F32(0.5)
        s = (((e[:, 0] + e[:, 1]) + e[:, 2]) + ((o[:, 0] + o[:, 1]) + o[:, 2])) * F32(0.5)
        m = np.where(s > 0, s, F32(0))
        err = (d / (F32(1e-4) + np.sqrt(m))).astype(F32)
    err = np.where((E_[:, 3] <= 0) | (O_[:, 3] <= 0), F32(np.inf), err)
    return F32(np.max(err))   # (NaN if any pixel's is)


def assert_ulps(got, want, n_ulps, what):
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    nan_g, nan_w = np.isnan(got), np.isnan(want)
    assert (nan_g == nan_w).all(), f"{what}: NaN at {np.argwhere(nan_g != nan_w).ravel()[:8].tolist()}"
    ok = ~nan_w
    assert (got[ok] >= 0).all() and (want[ok] >= 0).all()
    diff = np.abs(got[ok].view(np.int32).astype(np.int64) - want[ok].view(np.int32).astype(np.int64))   # (non-negative floats: bits are ordered)
    assert diff.max(initial=0) <= n_ulps, f"{what}: {diff.max()} ulps at {np.argwhere(ok).ravel()[np.argmax(diff)]}: {got[ok][np.argmax(diff)]} vs {want[ok][np.argmax(diff)]}"


def tiles_over(w, h):
    """every 8 x 8 tile that covers part of a w x h image, row by row (BlockQueue refuses sizes that are not multiples of 8; the error kernel
    takes any list and clips to the image)"""
    return np.array([(x, y) for y in range((h + 7) // 8) for x in range((w + 7) // 8)], np.uint32).reshape(-1, 2)


# ---- the GPU tests' helpers

def rgb(img):
    return img[..., :3] / np.maximum(img[..., 3:], 1e-20)


def rmse(a, b):
    return float(np.sqrt(np.mean((rgb(a) - rgb(b)) ** 2)))


def size(scene, frame):
    film = scene.flatten(frame).contents.film
    return film.width, film.height


def queue(scene, frame):
    return np.array(T.BlockQueue(size(scene, frame), (8, 8)).blocks, np.uint32).reshape(-1, 2)


def device_film(scene, hip, frame, spp, rng=None):
    """one launch into a zeroed device film: the samples rng of every tile (rng None: tray_render_tiles_device)"""
    import torch
    w, h = size(scene, frame)
    film = torch.zeros(w * h * 4, dtype=torch.float32, device="cuda:0")
    if rng is None:
        hip.render_device(scene, frame, (0, 0), spp, film.data_ptr())
    else:
        hip.render_samples_device(scene, frame, (0, 0), spp, rng, film.data_ptr())
    torch.cuda.synchronize()
    return film.cpu().numpy().reshape(h, w, 4)


def pixels_in_image(scene, frame, q):
    w, h = size(scene, frame)
    return np.array([min(8, w - 8 * int(x)) * min(8, h - 8 * int(y)) for x, y in q], np.int64)


def assert_close(got, want, what):
    scale = max(1.0, float(np.abs(want).max()))
    d = float(np.abs(got - want).max())
    print(f"{what}: max difference {d:.2e} (bar {2e-5 * scale:.2e})")
    assert d <= 2e-5 * scale, what


def load(d, tmp_path, name="s.json"):
    scenes.write_assets(str(tmp_path))
    p = os.path.join(str(tmp_path), name)
    with open(p, "w") as f:
        json.dump(d, f)
    return T.Scene.load_file(p)


def spheres_in_the_dark(width, height, samples):
    """smallpt without its walls: two spheres under the sphere light, the rest of the frame sees nothing"""
    d = scenes.smallpt(width, height, samples)
    d["objects"] = [o for o in d["objects"] if o["name"] != "walls"]
    for o in d["objects"]:
        if o["name"] == "metal_sphere":
            o["material"] = "white_wall"
    return d


def oracle_film(flat, q, n_t, spp, seed):
    """the oracle's RenderTarget::write of the samples [0, n_t[i]) of every pixel of tile q[i] (a spp-sample frame)"""
    fs = flat.contents
    w, h = fs.film.width, fs.film.height
    r = 6
    ref = np.zeros((h + 2 * r, w + 2 * r, 4), np.float32)
    for tile, n in zip(q, n_t):
        n = int(n)
        px, py = np.meshgrid(np.arange(8) + 8 * int(tile[0]), np.arange(8) + 8 * int(tile[1]))
        out = O.sample_radiance(flat, np.repeat(px.ravel(), n), np.repeat(py.ravel(), n), np.tile(np.arange(n), 64), spp, seed=seed)
        patches = O.film_patches(fs.film, (int(tile[0]), int(tile[1])), np.concatenate([out[:, 3:5], out[:, 0:3]], 1), r)
        for (x, y), p in zip(np.floor(out[:, 3:5]).astype(int), patches):
            ref[y:y + 2 * r + 1, x:x + 2 * r + 1] += p
    return ref[r:r + h, r:r + w]
