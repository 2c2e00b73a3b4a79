"""The numpy statements of what the filtered stopping rule adds (include/trayhip.h: tray_denoise_halves_device,
tray_render_noise_target_filtered_device), shared by the CPU and the GPU tests: the two cross-filtered halves of the dual-buffer filter, written
next to _denoise_ref.denoise in F = float32 or float64; the noise-target metric of a tile evaluated on the halves; the block list of a set of
active tiles; and the bar of a half, which is _denoise_ref.bar's rule applied to that half."""
import numpy as np

from _denoise_ref import EPS, F32, F64, box, resolve, shift

BW, BH = 32, 16   # TRAY_DENOISE_BLOCK_W / _H


def halves(E, O, r=7, f=3, k=0.45, F=F64):
    """(A, wA, B, wB): A, B (h, w, 3) in F, wA, wB (h, w) bool -- whether the half's denominator is > 0. The statement of
    _denoise_ref.denoise, whose output is (A + B) / 2."""
    valid, a, b = resolve(E, O, F)
    vm = valid.astype(F)
    v = ((a - b) * (a - b) * F(0.5)).astype(F)
    cnt = box(vm, 1)
    with np.errstate(all="ignore"):
        V = np.where(cnt[..., None] > 0, box(v, 1) / np.maximum(cnt, F(1))[..., None], F(0)).astype(F)
    k2 = F(F32(k)) * F(F32(k))
    eps = F(F32(EPS))
    out = []
    for x, y in ((b, a), (a, b)):   # weights from x, applied to y
        num = np.zeros_like(a)
        den = np.zeros(a.shape[:2], F)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                xq, Vq, mq = shift(x, dy, dx), shift(V, dy, dx), shift(vm, dy, dx)
                pair = vm * mq
                diff = x - xq
                with np.errstate(all="ignore"):
                    t = (diff * diff - (V + np.minimum(V, Vq))) / (eps + k2 * (V + Vq))
                    t = (t.sum(-1) * pair).astype(F)
                    n = box(pair, f)
                    d2 = np.where(n > 0, box(t, f) / (F(3) * np.maximum(n, F(1))), F(0))
                    wgt = (np.exp(-np.maximum(d2, F(0))).astype(F) * mq * (n > 0)).astype(F)
                num += wgt[..., None] * shift(y, dy, dx)
                den += wgt
        with np.errstate(all="ignore"):
            out += [np.where(den[..., None] > 0, num / den[..., None], F(0)).astype(F), den > 0]
    return tuple(out)


def assert_halves_match(fa, fb, E, O, r, f, k, what):
    """fa / fb (h, w, 4) of the kernels against the f64 statement: each half within 4 x the f32 statement's distance from the f64 one on that half,
    plus 1e-7 (_denoise_ref.bar's rule); the weights are those of the f32 statement exactly (they are decided by f32 arithmetic: exp underflows
    to 0 below -103.97 in f32), and where the f64 statement has no weight there is none; a half without weight is 0."""
    want = halves(E, O, r, f, k, F64)
    f32 = halves(E, O, r, f, k, F32)
    for name, got, i in (("A", np.asarray(fa), 0), ("B", np.asarray(fb), 2)):
        assert np.isfinite(got).all(), f"{what} {name}: non-finite output"
        assert (got[..., 3] == f32[i + 1].astype(F32)).all(), f"{what} {name}: weights differ at {np.argwhere(got[..., 3] != f32[i + 1])[:4].tolist()}"
        assert not (got[..., 3] != 0)[~want[i + 1]].any(), f"{what} {name}: a weight where the f64 statement has none"
        assert (got[..., :3][got[..., 3] == 0] == 0).all(), f"{what} {name}: a half without weight is not 0"
        err32 = float(np.abs(f32[i].astype(F64) - want[i]).max())
        diff = np.abs(got[..., :3].astype(F64) - want[i])
        print(f"{what} {name}: kernels - f64 statement = {diff.max():.3e}, f32 statement - f64 statement = {err32:.3e}, bar {4 * err32 + 1e-7:.3e}")
        assert diff.max() <= 4.0 * err32 + 1e-7, f"{what} {name}: {diff.max():.3e} > {4 * err32 + 1e-7:.3e} at {np.unravel_index(np.argmax(diff), diff.shape)}"


def tile_error(fa, fb, tile, F=F32):
    """include/trayhip.h's tile error on the halves as films (fa, fb) in F, the header's operations in its order: with w = 1 the quotients are
    the colours; a pixel of weight 0 in either half is +inf"""
    tx, ty = int(tile[0]), int(tile[1])
    E_ = fa[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8].reshape(-1, 4).astype(F)
    O_ = fb[8 * ty:8 * ty + 8, 8 * tx:8 * tx + 8].reshape(-1, 4).astype(F)
    with np.errstate(all="ignore"):
        e, o = E_[:, :3] / E_[:, 3:], O_[:, :3] / O_[:, 3:]
        d = ((np.abs(e[:, 0] - o[:, 0]) + np.abs(e[:, 1] - o[:, 1])) + np.abs(e[:, 2] - o[:, 2])) * F(0.5)
        s = (((e[:, 0] + e[:, 1]) + e[:, 2]) + ((o[:, 0] + o[:, 1]) + o[:, 2])) * F(0.5)
        m = np.where(s > 0, s, F(0))
        err = (d / (F(F32(1e-4)) + np.sqrt(m))).astype(F)
    err = np.where((E_[:, 3] <= 0) | (O_[:, 3] <= 0), F(np.inf), err)
    return F(np.max(err))


def blocks_of(width, height):
    return (width + BW - 1) // BW, (height + BH - 1) // BH


def block_list(tiles, active, width, height):
    """the 32 x 16 blocks that hold a tile (8 x 8 pixels, (x, y) in tiles) of `tiles` whose flag in `active` is set (None: all of them), as sorted
    row-major indices; tiles outside the frame's blocks are passed over"""
    bx, by = blocks_of(width, height)
    tiles = np.asarray(tiles, np.int64).reshape(-1, 2)
    keep = np.ones(len(tiles), bool) if active is None else np.asarray(active) != 0
    x, y = tiles[keep, 0] // (BW // 8), tiles[keep, 1] // (BH // 8)
    inside = (x < bx) & (y < by)
    return np.unique(y[inside] * bx + x[inside]).astype(np.uint32)


def block_mask(blocks, width, height):
    """the pixels (h, w) bool of the listed blocks"""
    bx, _ = blocks_of(width, height)
    mask = np.zeros((height, width), bool)
    for b in np.asarray(blocks, np.int64):
        x0, y0 = (b % bx) * BW, (b // bx) * BH
        mask[y0:y0 + BH, x0:x0 + BW] = True
    return mask


def block_lists(w, h):
    """the block lists the tests of a listed call go through, by name"""
    bx, by = blocks_of(w, h)
    n = bx * by
    rng = np.random.default_rng(w + h)
    last = sorted(set(range(bx - 1, n, bx)) | set(range((by - 1) * bx, n)))   # the last column and the last row
    return {"empty": [], "last-row-and-column": last, "all": list(range(n)), "scattered": sorted(rng.choice(n, max(1, n // 3), replace=False).tolist()),
            "unordered-with-one-outside": [n - 1, 0, n + 5]}
