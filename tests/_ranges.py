"""What the tests of sample ranges share (tests/test_sample_ranges_emu.py and the features built on range launches): the tile queue of an image,
the oracle's film of one range of samples, and the bars a range's film is held to. Nothing here builds or loads an emulation library."""
import numpy as np

import tray_rust_amd as T
import _oracle as O
from _emu import FILM_PATCH_R

SPP = 16   # the frame the range tests cut their ranges from
SEED = 7


def tile_queue(width, height):
    return np.array(T.BlockQueue((width, height), (8, 8)).blocks, np.uint32).reshape(-1, 2)


def oracle_range(flat, q, rng, spp=SPP, seed=SEED):
    """the oracle's film of the samples [begin, end) of every pixel of the tiles q (a spp-sample frame): oracle_sample_radiance for the samples
    (clamped colour, film position, vertices, rays), oracle_film_patches for RenderTarget::write of each; returns (rgbw image, (samples, vertices, rays))"""
    fs = flat.contents
    w, h = fs.film.width, fs.film.height
    r = FILM_PATCH_R
    pad = np.zeros((h + 2 * r, w + 2 * r, 4), np.float32)
    counts = np.zeros(3, np.int64)
    for tile in q:
        px, py = np.meshgrid(np.arange(8) + 8 * int(tile[0]), np.arange(8) + 8 * int(tile[1]))
        px, py = np.repeat(px.ravel(), rng[1] - rng[0]), np.repeat(py.ravel(), rng[1] - rng[0])
        si = np.tile(np.arange(rng[0], rng[1]), 64)
        out = O.sample_radiance(flat, px, py, si, spp, seed=seed)
        counts += (len(out), int(out[:, 5].sum()), int(out[:, 6].sum()))
        s = np.concatenate([out[:, 3:5], out[:, 0:3]], 1)
        patches = O.film_patches(fs.film, (int(tile[0]), int(tile[1])), s, r)
        for (x, y), p in zip(np.floor(out[:, 3:5]).astype(int), patches):
            pad[y:y + 2 * r + 1, x:x + 2 * r + 1] += p   # (patch pixel (r, r) is the sample's own pixel; pad shifts by r)
    return pad[r:r + h, r:r + w].copy(), tuple(int(c) for c in counts)


def assert_film_matches(img, ref, what):
    """touched pixels equal; weight per pixel within 2e-5 of the pixel's own weight (tests/test_film_footprints.py)"""
    t_img, t_ref = img[..., 3] != 0, ref[..., 3] != 0
    assert (t_img == t_ref).all(), f"{what}: touched pixels differ at {np.argwhere(t_img != t_ref)[:8].tolist()}"
    wr = np.abs(img[..., 3] - ref[..., 3])[t_ref] / np.abs(ref[..., 3][t_ref])
    assert wr.max() <= 2e-5, f"{what}: per-pixel relative weight difference {wr.max():.2e} on {int((wr > 2e-5).sum())} px"
    full = ref[..., 3] >= 0.1 * ref[..., 3].max()
    a = img[..., :3][full] / img[..., 3:][full]
    b = ref[..., :3][full] / ref[..., 3:][full]
    assert np.abs(a - b).max() < 2e-5, what
