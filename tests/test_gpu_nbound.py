"""The neighbour bound of the two noise-target calls on the GPU (tray_scene_set_noise_ratio, Hip.render_noise_target(max_ratio=...)).

The emulation's cases (tests/test_nbound_emu.py: cornell_box without its back wall, min_spp 2, max_spp 64) at 48 x 32 and 64 x 64 on the device.
The threshold leaves the call WITHOUT a bound a neighbouring pair 8x apart or more (asserted first). With ratio 2 and 4: every pair of
neighbours within the ratio, n_t a power of two in [min, max], the samples counted those of the reported n_t, even + odd equal to the sum over
the tiles of tray_render_samples_device's film of that tile's [0, n_t) (2e-5 of the film's largest value: both are f32 atomic sums of the same
splats in another order), and n_t equal to the emulation's -- the library's schedule over the emulated kernels, where a render is
tray_render_samples_device of the listed tiles, so that the emulated error kernel reads the device's films up to that rounding (no tile error
of any round may lie within 1e-3 of the threshold: choose another then). Ratio 0 gives the call's tile_samples and launches without the setter;
both schedules render the 64 x 64 case; the filtered rule runs under the bound; Hip.render_noise_target(max_ratio=...) is the C calls'."""
import ctypes as C

import numpy as np
import pytest

import tray_rust_amd as T
import _first_hit_ref as FH
import _nbound_ref as NB
from _noise_ref import assert_close, load, pixels_in_image, queue as queue_of

pytestmark = pytest.mark.gpu

LO, HI, SEED = 2, 64, 7
LEVELS = NB.levels_of(LO, HI)
THRESHOLD = {(48, 32): 0.6, (64, 64): 0.5}


def target(scene, hip, threshold, ratio=None, filt=None):
    """one noise-target call over the whole queue under tray_scene_set_noise_ratio(ratio) (None: the setter is not called); filt = (radius,
    patch, k): the filtered call. Returns (even, odd, tile_samples, tile_error, timing)."""
    import torch
    lib = T.lib()
    w, h = scene.flatten(0).contents.film.width, scene.flatten(0).contents.film.height
    dev = scene.device_scene(0, 0)
    spp = hip._select_sampler(dev, HI)
    even = torch.zeros(w * h * 4, dtype=torch.float32, device="cuda:0")
    odd = torch.zeros_like(even)
    n = len(queue_of(scene, 0))
    smp, err = np.zeros(n, np.uint32), np.zeros(n, np.float32)
    sp, ep = smp.ctypes.data_as(C.POINTER(C.c_uint32)), err.ctypes.data_as(C.POINTER(C.c_float))
    if ratio is not None:
        T.check(lib.tray_scene_set_noise_ratio(dev, ratio))
    try:
        if filt is None:
            T.check(lib.tray_render_noise_target_device(dev, 0, 0, LO, spp, float(threshold), hip.seed, C.c_void_p(even.data_ptr()), C.c_void_p(odd.data_ptr()),
                                                        sp, ep, None))
        else:
            scratch = torch.empty(int(lib.tray_noise_target_filtered_scratch_bytes(w, h)), dtype=torch.uint8, device="cuda:0")
            T.check(lib.tray_render_noise_target_filtered_device(dev, 0, 0, LO, spp, float(threshold), hip.seed, C.c_void_p(even.data_ptr()),
                                                                 C.c_void_p(odd.data_ptr()), filt[0], filt[1], filt[2], None, C.c_void_p(scratch.data_ptr()), sp,
                                                                 ep, None))
    finally:
        if ratio is not None:
            T.check(lib.tray_scene_set_noise_ratio(dev, 0))
    torch.cuda.synchronize()
    return even.cpu().numpy().reshape(h, w, 4), odd.cpu().numpy().reshape(h, w, 4), smp, err, hip.timing(scene)


class Pieces:
    """tray_render_samples_device's film of the samples [begin, end) of one tile of the queue, rendered once"""

    def __init__(self, scene, hip):
        self.scene, self.hip, self.cache = scene, hip, {}
        film = scene.flatten(0).contents.film
        self.w, self.h = film.width, film.height

    def __call__(self, i, begin, end):
        import torch
        if (i, begin, end) not in self.cache:
            film = torch.zeros(self.w * self.h * 4, dtype=torch.float32, device="cuda:0")
            self.hip.render_samples_device(self.scene, 0, (i, 1), HI, (begin, end), film.data_ptr())
            torch.cuda.synchronize()
            self.cache[i, begin, end] = film.cpu().numpy().reshape(self.h, self.w, 4)
        return self.cache[i, begin, end]


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    """size -> (scene, hip, queue, pieces, the call without a bound)"""
    out = {}
    for size in THRESHOLD:
        scene, *_ = load(FH.open_cornell(size[0], size[1], HI), tmp_path_factory.mktemp(f"nbound{size[0]}"))
        hip = T.Hip(0, seed=SEED)
        out[size] = (scene, hip, queue_of(scene, 0), Pieces(scene, hip), target(scene, hip, THRESHOLD[size]))
    return out


def emulated(queue, size, threshold, ratio, pieces):
    """the emulated call whose renders are the device's range launches; returns (n_t, the smallest relative distance of a tile error to the threshold)"""
    margins = []

    def render(B, sel, begin, end, film):
        for i in sel:
            film += pieces(int(i), begin, end)

    def after_read(B, n_words):
        e = B.err[np.isfinite(B.err)]
        if len(e):
            margins.append(float(np.abs(e - threshold).min() / threshold))

    rc, _, B = NB.target(queue, size[0], size[1], LO, HI, np.float32(threshold), ratio, render, after_read)
    assert rc == 0
    return B.samples.copy(), min(margins)


@pytest.mark.parametrize("ratio", [2, 4])
@pytest.mark.parametrize("size", list(THRESHOLD), ids=["48x32", "64x64"])
def test_bounded_call_on_the_device(cases, size, ratio):
    scene, hip, queue, pieces, (_, _, before, _, _) = cases[size]
    assert NB.worst_ratio(queue, before) >= 8, f"the unbounded call leaves no pair 8x apart ({before.tolist()}): the case checks nothing"
    even, odd, smp, err, tim = target(scene, hip, THRESHOLD[size], ratio)
    print(f"{size} ratio {ratio}: n_t {smp.tolist()}\n unbounded {before.tolist()}; samples {int(smp.sum())} against {int(before.sum())} per pixel of a tile")
    NB.assert_result(queue, smp, LO, HI, ratio, f"{size} ratio {ratio}")
    assert tim.samples == int((pixels_in_image(scene, 0, queue) * smp.astype(np.int64)).sum())
    assert (err[smp < HI] < THRESHOLD[size]).all(), "a tile stopped below max_spp with its last error not under the threshold"
    assert_close(even + odd, sum(pieces(i, 0, int(n)) for i, n in enumerate(smp)), f"{size} ratio {ratio}: even + odd against the tiles' [0, n_t)")
    want, margin = emulated(queue, size, THRESHOLD[size], ratio, pieces)
    assert margin > 1e-3, f"a tile's error lies within {margin:.1e} of the threshold {THRESHOLD[size]}: choose another"
    assert (smp == want).all(), f"n_t is not the emulation's: {smp.tolist()} against {want.tolist()}"


def test_ratio_zero_is_the_call_without_the_setter(cases):
    scene, hip, queue, _, (even0, odd0, before, err0, tim0) = cases[(64, 64)]
    launches0 = tim0.launches
    even, odd, smp, err, tim = target(scene, hip, THRESHOLD[(64, 64)], 0)
    assert (smp == before).all() and tim.launches == launches0 == 4 * (int(np.log2(int(before.max()) // LO)) + 1)
    assert_close(even + odd, even0 + odd0, "ratio 0 against the call without the setter")


@pytest.mark.parametrize("mode", ["mega", "wave"])
def test_both_schedules(mode, tmp_path, monkeypatch):
    monkeypatch.setenv("TRAYHIP_MODE", mode)
    scene, *_ = load(FH.open_cornell(64, 64, HI), tmp_path)
    hip = T.Hip(0, seed=SEED)
    queue = queue_of(scene, 0)
    even, odd, smp, err, tim = target(scene, hip, THRESHOLD[(64, 64)], 4)
    assert hip.schedule(scene)["launched_wavefront"] == (1 if mode == "wave" else 0), "TRAYHIP_MODE did not select the schedule"
    NB.assert_result(queue, smp, LO, HI, 4, mode)
    assert tim.samples == int((pixels_in_image(scene, 0, queue) * smp.astype(np.int64)).sum())
    pieces = Pieces(scene, hip)
    assert_close(even + odd, sum(pieces(i, 0, int(n)) for i, n in enumerate(smp)), f"{mode}: even + odd against the tiles' [0, n_t)")


def test_filtered_rule_under_the_bound(cases):
    scene, hip, queue, pieces, _ = cases[(48, 32)]
    *_, before, _, _ = target(scene, hip, 0.2, None, (7, 3, 0.45))
    assert NB.worst_ratio(queue, before) >= 8, before.tolist()
    even, odd, smp, err, tim = target(scene, hip, 0.2, 4, (7, 3, 0.45))
    NB.assert_result(queue, smp, LO, HI, 4, "filtered")
    assert_close(even + odd, sum(pieces(i, 0, int(n)) for i, n in enumerate(smp)), "filtered: even + odd against the tiles' [0, n_t)")


def test_no_pixel_weight_below_the_bound_the_ratio_guarantees(cases):
    """The weight check. A pixel p of tile t gets w(p) = sum over the camera samples s of f(p, s), f the film's filter table as RenderTarget::write
    looks it up (_nbound_ref.filter_bounds). The samples come pixel by pixel: pixel q of tile u holds n_u of them, somewhere in its square (a
    prefix of the frame's shuffled low-discrepancy sequence is not stratified, so nothing better is known about where), and each adds at least
    least(p - q), the smallest table entry a position in q's square can reach at p. The pixels of p's own tile hold exactly n_t samples each; a
    pixel of another tile in the filter's reach belongs to a neighbour of t, which under ratio R holds at most R n_t, and what it adds is at
    least R n_t min(least, 0). So
        w(p) >= n_t (sum over q in t of least(p - q) + R sum over q outside t of min(least(p - q), 0)),
    pixels outside the image left out (they hold no samples). Asserted for the bounded films, and violated by the unbounded ones' construction
    only if a neighbour is more than R ahead. For Mitchell-Netravali at width 2 this bound is NEGATIVE for every R, even 1: the pixel's own
    samples guarantee 0.215 n_t (the table at the pixel's corner) and the worst positions of its neighbours' take 0.43 n_t away -- a worst case no
    render comes near. The same sum over the table's MEAN per pixel square, what a sample adds on average, is positive at a tile's corner pixel
    while R < 33: 0.770 n_t of its own tile against 0.0233 R n_t ("Rendering to a noise threshold"); that one is an expectation, so it
    is printed, not asserted."""
    scene, hip, queue, _, (even0, odd0, before, _, _) = cases[(64, 64)]
    film = scene.flatten(0).contents.film
    even, odd, smp, err, tim = target(scene, hip, THRESHOLD[(64, 64)], 4)
    w = (even + odd)[..., 3].astype(np.float64)
    floor, mean_floor = NB.weight_floor(film, queue, smp, 4), NB.weight_floor(film, queue, smp, 4, kind=1)
    slack = 2e-5 * np.abs(w).max()   # (the f32 sums)
    print(f"ratio 4: min w {w.min():.3f}; the bound's largest value {floor.max():.3f}; pixels under the mean bound {int((w < mean_floor).sum())} of {w.size}; "
          f"unbounded: min w {(even0 + odd0)[..., 3].min():.3f}")
    assert (w >= floor - slack).all(), f"{int((w < floor - slack).sum())} pixels below the bound"
    least, mean = NB.filter_bounds(film)
    assert least.sum() < 0 < least[4, 4] and mean_floor.min() > 0   # what the docstring and DESIGN.md say of the two bounds
    assert w.min() > 0, "a pixel without weight in the bounded films"


def test_python_max_ratio(cases, tmp_path):
    scene, hip, queue, _, _ = cases[(64, 64)]
    _, rt, _, fi = load(FH.open_cornell(64, 64, HI), tmp_path)
    cfg = T.Config(".", "s", HI, 1, fi, (0, 0))
    rt.clear()
    smp, err = hip.render_noise_target(scene, rt, cfg, THRESHOLD[(64, 64)], min_spp=LO, max_ratio=4)
    even, odd, smp_c, _, _ = target(scene, hip, THRESHOLD[(64, 64)], 4)
    assert (smp == smp_c).all() and NB.worst_ratio(queue, smp) <= 4
    assert_close(rt.get_renderf32().reshape(64, 64, 4), even + odd, "render_noise_target(max_ratio=4) against the C call's films")
    # the device scene is back at ratio 0
    *_, smp0, _, _ = target(scene, hip, THRESHOLD[(64, 64)])
    assert NB.worst_ratio(queue, smp0) >= 8
    with pytest.raises(ValueError):
        hip.render_denoised(scene, rt, cfg, max_ratio=4)
    with pytest.raises(T.TrayError):
        hip.render_noise_target(scene, rt, cfg, 0.5, min_spp=LO, max_ratio=3)
