"""The dual-buffer NL-means filter of tray_denoise_device (include/trayhip.h) as a numpy statement, typed: denoise(E, O, r, f, k, F) evaluates
it in F = np.float32 (the arithmetic the kernels do, in numpy's order of summation) or F = np.float64 (what the tests compare with). Also the
test films, the bar of the comparisons and the range property, shared by the CPU and the GPU tests of the denoiser, and the GPU tests' one call
of tray_denoise_device between guard bytes and their many-sample reference image (torch is imported there, where a GPU is used)."""
import ctypes as C

import numpy as np

import tray_rust_amd as T

F32, F64 = np.float32, np.float64
EPS = 1e-7


def shift(img, dy, dx):
    """img[y + dy, x + dx] at (y, x), 0 outside"""
    h, w = img.shape[:2]
    out = np.zeros_like(img)
    ys0, ys1 = max(0, -dy), min(h, h - dy)
    xs0, xs1 = max(0, -dx), min(w, w - dx)
    if ys0 < ys1 and xs0 < xs1:
        out[ys0:ys1, xs0:xs1] = img[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx]
    return out


def box(img, f):
    """the sum of the (2f+1)^2 shifts"""
    out = np.zeros_like(img)
    for dy in range(-f, f + 1):
        for dx in range(-f, f + 1):
            out = out + shift(img, dy, dx)
    return out


def resolve(E, O, F=F32):
    """(valid, a, b) of two RGBW films: validity is decided on the films as given (float32), the quotients are taken in F"""
    with np.errstate(all="ignore"):
        valid = (E[..., 3] > 0) & (O[..., 3] > 0) & np.isfinite(E).all(-1) & np.isfinite(O).all(-1)
        E_, O_ = E.astype(F), O.astype(F)
        a = np.where(valid[..., None], E_[..., :3] / E_[..., 3:], F(0)).astype(F)
        b = np.where(valid[..., None], O_[..., :3] / O_[..., 3:], F(0)).astype(F)
    return valid, a, b


def denoise(E, O, r=7, f=3, k=0.45, F=F64, min_foreign_d2=None):
    """out (h, w, 3) of the filter in F. k is the float32 the ABI takes. min_foreign_d2: a one-element list that receives the smallest d2 of
    any offset other than (0, 0) with a non-empty patch (the noise-free property checks it)."""
    valid, a, b = resolve(E, O, F)
    vm = valid.astype(F)
    v = ((a - b) * (a - b) * F(0.5)).astype(F)
    cnt = box(vm, 1)
    with np.errstate(all="ignore"):
        V = np.where(cnt[..., None] > 0, box(v, 1) / np.maximum(cnt, F(1))[..., None], F(0)).astype(F)
    k2 = F(F32(k)) * F(F32(k))
    eps = F(F32(EPS))
    outs = []
    lowest = np.inf
    for x, y in ((b, a), (a, b)):   # weights from x, applied to y
        num = np.zeros_like(a)
        den = np.zeros(a.shape[:2], F)
        for dy in range(-r, r + 1):
            for dx in range(-r, r + 1):
                xq, Vq, mq = shift(x, dy, dx), shift(V, dy, dx), shift(vm, dy, dx)
                pair = vm * mq   # both pixels valid and inside
                diff = x - xq
                with np.errstate(all="ignore"):
                    t = (diff * diff - (V + np.minimum(V, Vq))) / (eps + k2 * (V + Vq))
                    t = (t.sum(-1) * pair).astype(F)
                    n = box(pair, f)
                    d2 = np.where(n > 0, box(t, f) / (F(3) * np.maximum(n, F(1))), F(0))
                    wgt = (np.exp(-np.maximum(d2, F(0))).astype(F) * mq * (n > 0)).astype(F)
                if (dy or dx) and (n > 0).any():
                    lowest = min(lowest, float(d2[n > 0].min()))
                num += wgt[..., None] * shift(y, dy, dx)
                den += wgt
        with np.errstate(all="ignore"):
            outs.append(np.where(den[..., None] > 0, num / den[..., None], F(0)).astype(F))
    if min_foreign_d2 is not None:
        min_foreign_d2.append(lowest)
    return ((outs[0] + outs[1]) * F(0.5)).astype(F)


def bar(E, O, r, f, k):
    """(want, tolerance, err32, f32): the f64 statement; 4 x the max abs difference of the f32 statement from it, plus 1e-7 -- the factor because
    the kernel sums the patch terms and the weights in another order than numpy --; that difference; the f32 statement"""
    want = denoise(E, O, r, f, k, F64)
    f32 = denoise(E, O, r, f, k, F32)
    err32 = float(np.abs(f32.astype(F64) - want).max())
    return want, 4.0 * err32 + 1e-7, err32, f32


def assert_matches(got_rgbw, E, O, r, f, k, what):
    """got (h, w, 4) of the kernels against the f64 statement under bar(); weight 1 everywhere; finite; the pixels of rgb == 0 as sets: those of
    the f32 statement exactly, which include those of the f64 one. (The two statements' sets differ where f32 arithmetic itself decides: exp
    underflows to 0 below -103.97 in f32 and below -745 in f64, so a pixel whose every candidate lies further than that -- an invalid pixel
    whose few partners sit across an edge -- has denominator 0 and output 0 in f32 and a mean of vanishing weights in f64.)"""
    want, tol, err32, f32 = bar(E, O, r, f, k)
    got = np.asarray(got_rgbw)
    assert np.isfinite(got).all(), f"{what}: non-finite output at {np.argwhere(~np.isfinite(got))[:4].tolist()}"
    assert (got[..., 3] == 1.0).all(), f"{what}: an output weight is not 1"
    diff = np.abs(got[..., :3].astype(F64) - want)
    print(f"{what}: kernels - f64 statement = {diff.max():.3e}, f32 statement - f64 statement = {err32:.3e}, bar {tol:.3e}")
    zero_g, zero_w, zero_64 = (got[..., :3] == 0).all(-1), (f32 == 0).all(-1), (want == 0).all(-1)
    assert (zero_g == zero_w).all(), f"{what}: the pixels with rgb == 0 differ at {np.argwhere(zero_g != zero_w)[:4].tolist()}"
    assert zero_g[zero_64].all(), f"{what}: a pixel the f64 statement leaves 0 is not 0 at {np.argwhere(zero_64 & ~zero_g)[:4].tolist()}"
    assert diff.max() <= tol, f"{what}: {diff.max():.3e} > {tol:.3e} at {np.unravel_index(np.argmax(diff), diff.shape)}"
    # The same bar over the valid pixels alone, whose denominators are >= 1: where an invalid pixel's weights are all denormal the f32 statement
    # itself is far from the f64 one, and the bar over the whole image, taken from that pixel, would say little about the others.
    valid = resolve(E, O)[0]
    if valid.any():
        err_v = float(np.abs(f32.astype(F64) - want)[valid].max())
        print(f"{what}: over the valid pixels {diff[valid].max():.3e}, f32 statement {err_v:.3e}")
        assert diff[valid].max() <= 4.0 * err_v + 1e-7, f"{what}: valid pixels: {diff[valid].max():.3e} > {4.0 * err_v + 1e-7:.3e}"
    return float(diff.max()), err32


def random_films(w, h, seed):
    """even / odd RGBW films of a smooth-ish image under noise, whose weights vary, with pixels of zero, negative and NaN weight, a NaN colour,
    pixels whose halves agree exactly, a valid pixel whose 3 x 3 box is otherwise invalid and (where the image has room) an 8 x 9 block of
    invalid pixels: larger than a patch"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([0.5 + 0.4 * np.sin(xx / 5.0 + c) * np.cos(yy / 7.0 - c) + (xx > w // 2) * 0.3 * c for c in range(3)], -1)
    films = []
    for _ in range(2):
        wgt = rng.uniform(0.5, 8.0, (h, w)).astype(F32)
        col = (base * rng.uniform(0.8, 1.2, (h, w, 3))).astype(F32)
        films.append(np.concatenate([col * wgt[..., None], wgt[..., None]], -1).astype(F32))
    even, odd = films
    n = w * h
    pick = lambda m: np.unravel_index(rng.choice(n, m, replace=False), (h, w))
    even[pick(min(3, n // 5))] = 0.0                     # no sample landed
    odd[pick(min(2, n // 7))] *= -1.0                    # negative weight
    ys, xs = pick(1); even[ys, xs, 1] = np.nan          # a NaN colour
    ys, xs = pick(1); odd[ys, xs, 3] = np.nan           # a NaN weight
    ys, xs = pick(min(4, n // 4)); odd[ys, xs] = even[ys, xs]   # both halves agree
    if w >= 5 and h >= 3:                               # a valid pixel alone in its 3 x 3 box
        cy, cx = h - 2, w - 3
        keep_e, keep_o = np.abs(even[cy, cx]) + F32(0.25), np.abs(odd[cy, cx]) + F32(0.25)   # (whatever was picked above: valid again)
        keep_e[~np.isfinite(keep_e)] = 1.0; keep_o[~np.isfinite(keep_o)] = 1.0
        even[cy - 1:cy + 2, cx - 1:cx + 2, 3] = 0.0
        even[cy, cx], odd[cy, cx] = keep_e, keep_o
    if w >= 20 and h >= 12:                             # a block of invalid pixels larger than a 7 x 7 patch
        odd[1:10, 2:10, 3] = 0.0
    return np.ascontiguousarray(even), np.ascontiguousarray(odd)


def range_violations(out_rgb, E, O, r, where=None):
    """the range property: every output channel lies between the minimum and the maximum of that channel of a and b over the valid pixels of
    the pixel's window, up to (2 (2r+1)^2 + 4) 2^-24 times the largest magnitude there. It is a property of a normalised sum, so it holds
    where both denominators are positive: at every valid pixel (its own weight is exp(-max(0, d2(p, p))) = 1, as t(p', p') <= 0), which is
    the default `where`; an invalid pixel has a positive denominator only if some q shares a valid patch position with it (never at
    patch 0) at a distance below exp's underflow. Returns the pixels (y, x) of `where` that break it."""
    valid, a, b = resolve(E, O, F32)
    h, w = valid.shape
    slack = (2 * (2 * r + 1) ** 2 + 4) * 2.0 ** -24
    lo = np.where(valid[..., None], np.minimum(a, b), np.inf).astype(F64)
    hi = np.where(valid[..., None], np.maximum(a, b), -np.inf).astype(F64)
    wlo, whi = np.full((h, w, 3), np.inf), np.full((h, w, 3), -np.inf)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ys0, ys1, xs0, xs1 = max(0, -dy), min(h, h - dy), max(0, -dx), min(w, w - dx)
            if ys0 < ys1 and xs0 < xs1:
                wlo[ys0:ys1, xs0:xs1] = np.minimum(wlo[ys0:ys1, xs0:xs1], lo[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx])
                whi[ys0:ys1, xs0:xs1] = np.maximum(whi[ys0:ys1, xs0:xs1], hi[ys0 + dy:ys1 + dy, xs0 + dx:xs1 + dx])
    none = ~np.isfinite(wlo)   # no valid pixel in the window: the output is 0
    wlo, whi = np.where(none, 0.0, wlo), np.where(none, 0.0, whi)
    mag = np.maximum(np.abs(wlo), np.abs(whi))
    o = np.asarray(out_rgb, F64)
    bad = (o < wlo - slack * mag) | (o > whi + slack * mag)
    return np.argwhere(bad.any(-1) & (valid if where is None else np.asarray(where, bool)))


def rgb(img):
    with np.errstate(all="ignore"):
        return np.where(img[..., 3:] > 0, img[..., :3] / img[..., 3:], 0).astype(F32)


def rmse(a, b):
    return float(np.sqrt(np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)))


# ---- on the GPU

GPU_GUARD = 4096   # bytes


def denoise_guarded(even, odd, r, f, k):
    """one tray_denoise_device call on films uploaded from the host, its output and scratch buffer between guard bytes; returns (h, w, 4)"""
    import torch
    GUARD = GPU_GUARD
    h, w = even.shape[:2]
    lib = T.lib()
    e, o = torch.from_numpy(np.ascontiguousarray(even)).cuda(), torch.from_numpy(np.ascontiguousarray(odd)).cuda()
    nb = int(lib.tray_denoise_scratch_bytes(w, h))
    assert nb > 0
    scr = torch.full((nb + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = torch.full((w * h * 16 + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    T.check(lib.tray_init(0))
    T.check(lib.tray_denoise_device(w, h, C.c_void_p(e.data_ptr()), C.c_void_p(o.data_ptr()), r, f, k, C.c_void_p(out.data_ptr() + GUARD),
                                    C.c_void_p(scr.data_ptr() + GUARD), None))
    torch.cuda.synchronize()
    assert (scr[:GUARD] == 0xA5).all() and (scr[GUARD + nb:] == 0xA5).all(), "a write outside tray_denoise_scratch_bytes of scratch"
    assert (out[:GUARD] == 0xA5).all() and (out[GUARD + w * h * 16:] == 0xA5).all(), "a write outside out_dev"
    assert (e.cpu().numpy().view(np.uint32) == even.view(np.uint32)).all() and (o.cpu().numpy().view(np.uint32) == odd.view(np.uint32)).all()
    return out[GUARD:GUARD + w * h * 16].view(torch.float32).reshape(h, w, 4).cpu().numpy()


def reference_image(scene, spp, seed):
    import torch
    fl = scene.flatten(0).contents.film
    film = torch.zeros(fl.width * fl.height * 4, dtype=torch.float32, device="cuda:0")
    T.Hip(0, seed=seed).render_device(scene, 0, (0, 0), spp, film.data_ptr())
    torch.cuda.synchronize()
    return rgb(film.cpu().numpy().reshape(fl.height, fl.width, 4))
