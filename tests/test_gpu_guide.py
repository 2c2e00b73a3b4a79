"""The filtered stopping rule on the GPU: tray_denoise_halves_device, tray_render_noise_target_filtered_device, Hip.denoise_halves and
error="filtered" of Hip.render_noise_target / Hip.render_denoised.

The halves against the f64 numpy statement (tests/_guide_ref.py) under _denoise_ref.bar's rule applied to each half, equal to
tray_denoise_device's output bit for bit when averaged, the same bits in two calls, guard bytes intact, block lists computing the listed blocks
only. The call: at threshold 0 every tile takes max_spp and even + odd is tray_render_tiles_device's film (the bar of
tests/test_gpu_noise_target.py), on the tile kernel and on the wavefront schedule; at a huge threshold every tile stops at min_spp; at a real
threshold the films are the oracle's film of each tile's [0, n_t), the errors of the last round's tiles are the numpy metric of the halves of the
returned films, and out_dev is a separate tray_denoise_device call's output; background tiles stop at min_spp with error 0; a 1920 x 1080
frame. Nothing here reads the reference."""
import ctypes as C

import numpy as np
import pytest

import tray_rust_amd as T
from tray_rust_amd import scenes
import _denoise_ref as D
import _guide_ref as G
import _noise_ref as NT
from _denoise_ref import GPU_GUARD as GUARD, denoise_guarded, reference_image
from _noise_ref import assert_ulps

pytestmark = pytest.mark.gpu

F32 = np.float32
RF = [(1, 0), (3, 1), (7, 3), (10, 3)]
R_, F_, K_ = 7, 3, 0.45


def halves_guarded(even, odd, r, f, k, blocks=None, fill=0xA5):
    """one tray_denoise_halves_device call on films uploaded from the host; fa, fb and the scratch buffer lie between guard bytes and are filled
    with `fill` bytes beforehand; returns (fa, fb) as (h, w, 4)"""
    import torch
    h, w = even.shape[:2]
    lib = T.lib()
    e, o = torch.from_numpy(np.ascontiguousarray(even)).cuda(), torch.from_numpy(np.ascontiguousarray(odd)).cuda()
    nb = int(lib.tray_denoise_scratch_bytes(w, h))
    scr = torch.full((nb + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    outs = [torch.full((w * h * 16 + 2 * GUARD,), fill, dtype=torch.uint8, device="cuda") for _ in range(2)]
    bl = None if blocks is None else torch.from_numpy(np.array(list(blocks) + [0], np.uint32).view(np.int32)).cuda()   # (never an empty allocation)
    T.check(lib.tray_init(0))
    T.check(lib.tray_denoise_halves_device(w, h, C.c_void_p(e.data_ptr()), C.c_void_p(o.data_ptr()), r, f, k,
                                           None if bl is None else C.c_void_p(bl.data_ptr()), 0 if bl is None else len(blocks),
                                           C.c_void_p(outs[0].data_ptr() + GUARD), C.c_void_p(outs[1].data_ptr() + GUARD),
                                           C.c_void_p(scr.data_ptr() + GUARD), None))
    torch.cuda.synchronize()
    assert (scr[:GUARD] == 0xA5).all() and (scr[GUARD + nb:] == 0xA5).all(), "a write outside tray_denoise_scratch_bytes of scratch"
    for out in outs:
        assert (out[:GUARD] == fill).all() and (out[GUARD + w * h * 16:] == fill).all(), "a write outside fa_dev / fb_dev"
    assert (e.cpu().numpy().view(np.uint32) == even.view(np.uint32)).all() and (o.cpu().numpy().view(np.uint32) == odd.view(np.uint32)).all()
    return tuple(out[GUARD:GUARD + w * h * 16].view(torch.float32).reshape(h, w, 4).cpu().numpy() for out in outs)


@pytest.mark.parametrize("r,f", RF, ids=[f"r{r}f{f}" for r, f in RF])
@pytest.mark.parametrize("w,h", [(67, 45), (160, 96)], ids=["67x45", "160x96"])
def test_halves_of_generator_films(built, w, h, r, f):
    even, odd = D.random_films(w, h, seed=11 * w + h)
    fa, fb = halves_guarded(even, odd, r, f, 0.45)
    G.assert_halves_match(fa, fb, even, odd, r, f, 0.45, f"gpu {w}x{h} r={r} f={f}")
    again = halves_guarded(even, odd, r, f, 0.45)
    assert (fa.view(np.uint32) == again[0].view(np.uint32)).all() and (fb.view(np.uint32) == again[1].view(np.uint32)).all(), "two calls differ"
    out = denoise_guarded(even, odd, r, f, 0.45)
    mean = ((fa[..., :3] + fb[..., :3]) * F32(0.5)).astype(F32)
    assert (mean.view(np.uint32) == out[..., :3].view(np.uint32)).all(), "(fa + fb) * 0.5 is not tray_denoise_device's output to the bit"
    pa, pb = T.Hip(0).denoise_halves(even, odd, r, f, 0.45)
    assert isinstance(pa, np.ndarray) and (pa.view(np.uint32) == fa.view(np.uint32)).all() and (pb.view(np.uint32) == fb.view(np.uint32)).all()


@pytest.mark.parametrize("w,h", [(67, 45), (160, 96)], ids=["67x45", "160x96"])
def test_block_lists(built, w, h):
    even, odd = D.random_films(w, h, seed=3 * w + h)
    full = halves_guarded(even, odd, R_, F_, K_)
    bx, by = G.blocks_of(w, h)
    for which, blocks in G.block_lists(w, h).items():
        got = halves_guarded(even, odd, R_, F_, K_, blocks=blocks, fill=0x5A)
        mask = G.block_mask([b for b in blocks if b < bx * by], w, h)   # (an index outside the frame's blocks is passed over)
        for g, want in zip(got, full):
            assert (g.view(np.uint32)[mask] == want.view(np.uint32)[mask]).all(), f"{which}: a listed block differs from the full run"
            assert (g.view(np.uint32)[~mask] == 0x5A5A5A5A).all(), f"{which}: a pixel outside the listed blocks was written"


def test_emulation_and_gpu_bits(built):
    """a finding, not a requirement: with tr::ref_expf on both sides and IEEE division the host emulation is expected to give the GPU's bits"""
    import _emu_features as EF   # (builds the emulation of the guide kernels when called, here only)
    even, odd = D.random_films(67, 45, seed=5)
    emu = EF.guide_lib()
    for r, f in RF:
        gpu = halves_guarded(even, odd, r, f, 0.45)
        cpu = EF.guide_halves(emu, even, odd, r, f, 0.45)
        for name, g, c in (("fa", gpu[0], cpu[0]), ("fb", gpu[1], cpu[1])):
            n = int((g.view(np.uint32) != c.view(np.uint32)).sum())
            print(f"r={r} f={f} {name}: {n} of {g.size} words differ between the host emulation and the GPU (max abs {np.abs(g - c).max():.3e})")
            assert np.abs(g - c).max() <= 1e-5


def filtered_target(scene, hip, frame, min_spp, max_spp, threshold, r=R_, f=F_, k=K_, with_out=False):
    """one tray_render_noise_target_filtered_device call over the whole queue, its scratch between guard bytes; returns (even, odd, tile_samples,
    tile_error, timing, out or None)"""
    import torch
    w, h = NT.size(scene, frame)
    dev = scene.device_scene(frame, 0)
    spp = hip._select_sampler(dev, max_spp)
    even = torch.zeros(w * h * 4, dtype=torch.float32, device="cuda:0")
    odd = torch.zeros_like(even)
    out = torch.zeros_like(even) if with_out else None
    nb = int(T.lib().tray_noise_target_filtered_scratch_bytes(w, h))
    assert nb >= w * h * 80
    scr = torch.full((nb + 2 * GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    n = len(NT.queue(scene, frame))
    smp, err = np.zeros(n, np.uint32), np.zeros(n, np.float32)
    T.check(T.lib().tray_render_noise_target_filtered_device(dev, 0, 0, min_spp, spp, float(threshold), hip.seed, C.c_void_p(even.data_ptr()),
                                                             C.c_void_p(odd.data_ptr()), r, f, k, C.c_void_p(out.data_ptr()) if with_out else None,
                                                             C.c_void_p(scr.data_ptr() + GUARD), smp.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                             err.ctypes.data_as(C.POINTER(C.c_float)), None))
    torch.cuda.synchronize()
    assert (scr[:GUARD] == 0xA5).all() and (scr[GUARD + nb:] == 0xA5).all(), "a write outside the scratch buffer"
    film = lambda t: t.cpu().numpy().reshape(h, w, 4)
    return film(even), film(odd), smp, err, hip.timing(scene), film(out) if with_out else None


def launches_of(smp, min_spp, with_out, per_range=1):
    """the launches of a call from its rounds: the first block list (2), per round two range launches, the filter's three, the error, the tile
    compaction and the block list's two, and tray_denoise_device's three at the end"""
    rounds = int(np.log2(int(smp.max()) // min_spp)) + 1
    return 2 + rounds * (2 * per_range + 7) + (3 if with_out else 0)


@pytest.mark.parametrize("mode", ["", "wave"], ids=["tile-kernel", "wavefront"])
def test_threshold_zero(mode, tmp_path, monkeypatch):
    if mode:
        monkeypatch.setenv("TRAYHIP_MODE", mode)
    scene, *_ = NT.load(scenes.cornell_box(64, 64, 32), tmp_path)
    hip = T.Hip(0, seed=3)
    even, odd, smp, err, tim, _ = filtered_target(scene, hip, 0, 4, 32, 0.0)
    assert hip.schedule(scene)["launched_wavefront"] == (1 if mode else 0), "TRAYHIP_MODE did not select the schedule"
    assert (smp == 32).all(), np.unique(smp)
    assert tim.samples == 64 * 64 * 32
    if not mode:
        assert tim.launches == launches_of(smp, 4, False)
    NT.assert_close(even + odd, NT.device_film(scene, hip, 0, 32), f"{mode or 'tiles'}: even + odd against tray_render_tiles_device")


def test_huge_threshold_stops_every_tile_at_min_spp(tmp_path):
    scene, *_ = NT.load(scenes.cornell_box(64, 64, 64), tmp_path)
    hip = T.Hip(0, seed=4)
    even, odd, smp, err, tim, _ = filtered_target(scene, hip, 0, 8, 64, 3.0e38)
    assert (smp == 8).all() and np.isfinite(err).all()
    assert tim.samples == 64 * 64 * 8 and tim.launches == launches_of(smp, 8, False) == 11
    NT.assert_close(even + odd, NT.device_film(scene, hip, 0, 64, (0, 8)), "huge threshold against [0, 8)")
    NT.assert_close(even, NT.device_film(scene, hip, 0, 64, (0, 4)), "even film against [0, 4)")


def test_a_real_threshold(tmp_path):
    w, h = 160, 96
    lo, hi, thr = 2, 32, 0.2
    scene, *_ = NT.load(scenes.cornell_box(w, h, hi), tmp_path)
    flat = scene.flatten(0)
    hip = T.Hip(0, seed=7)
    even, odd, smp, err, tim, out = filtered_target(scene, hip, 0, lo, hi, thr, with_out=True)
    q = NT.queue(scene, 0)
    print(f"{w}x{h}: samples per tile {np.unique(smp, return_counts=True)}, launches {tim.launches}")
    assert all(lo <= n <= hi and (n & (n - 1)) == 0 for n in smp)
    assert len(np.unique(smp)) > 1, "the threshold decides nothing on this frame"
    assert (err[smp < hi] < thr).all()
    assert tim.samples == int((64 * smp.astype(np.int64)).sum())
    assert tim.launches == launches_of(smp, lo, True)
    # the films are the oracle's film of exactly each tile's [0, n_t) (the bars of tests/test_gpu_noise_target.py)
    img = even + odd
    ref = NT.oracle_film(flat, q, smp, hi, 7)
    t_img, t_ref = img[..., 3] != 0, ref[..., 3] != 0
    assert (t_img == t_ref).all()
    wr = np.abs(img[..., 3] - ref[..., 3])[t_ref] / ref[..., 3][t_ref]
    assert wr.max() <= 2e-5, wr.max()
    assert NT.rmse(img, ref) < 1e-4
    # the tiles of the call's last round: their error was taken from the halves of the returned films
    fa, fb = halves_guarded(even, odd, R_, F_, K_)
    last = smp == smp.max()
    assert_ulps(err[last], np.array([G.tile_error(fa, fb, t) for t in q[last]], F32), 4, f"{w}x{h} errors of the last round's tiles")
    # out_dev is a separate tray_denoise_device call on the returned films
    sep = denoise_guarded(even, odd, R_, F_, K_)
    assert (out.view(np.uint32) == sep.view(np.uint32)).all(), "out_dev differs from a separate tray_denoise_device call"


@pytest.mark.parametrize("rule", ["raw", "filtered"])
def test_the_launches_are_the_plans(rule, tmp_path):
    """the launches TrayKernelTiming counts are those the plan's schedule (noise_plan.h, through the recording Ops of tests/emu/noise_plan_record.h)
    makes when its count reads are answered as this call's were: after the round to `taken` samples a tile is active iff its n_t is larger"""
    import _noise_plan as NP   # (loads the emulation library of the guide kernels, which has the plan's exports)
    w, h, lo, hi, thr = 64, 48, 8, 64, 0.2
    scene, *_ = NT.load(scenes.cornell_box(w, h, hi), tmp_path)
    hip = T.Hip(0, seed=5)
    q = NT.queue(scene, 0)
    if rule == "raw":
        import test_gpu_noise_target as RAW
        *_, smp, err, tim = RAW.noise_target(scene, hip, 0, lo, hi, thr)
    else:
        *_, smp, err, tim, _ = filtered_target(scene, hip, 0, lo, hi, thr, with_out=True)
    script = [] if rule == "raw" else [len(G.block_list(q, None, w, h))]
    for taken in (8, 16, 32, 64):
        active = (smp > taken).astype(np.uint32)
        script += [int(active.sum())] + ([] if rule == "raw" else [len(G.block_list(q, active, w, h))])
    events, rc, launches = NP.record(rule == "filtered", True, w, h, len(q), len(q), lo, hi, script)   # (one launch per render: a static scene's tile kernel)
    print(f"{rule}: samples per tile {np.unique(smp, return_counts=True)}, {tim.launches} launches, the plan's {launches}")
    assert rc == 0 and tim.launches == launches
    assert tim.samples == 64 * sum(a["n"] * (a["end"] - a["begin"]) for g, a in events if g == "render")   # the ranges the plan lists are the samples taken


def test_background_tiles_stop_at_min_spp(tmp_path):
    """tiles farther than the reconstruction filter's radius plus the denoiser's window from any geometry see 0 in both films and in both
    halves: error 0, so they stop after round 0; tiles on the lit spheres take more samples"""
    scene, *_ = NT.load(NT.spheres_in_the_dark(96, 96, 128), tmp_path)
    hip = T.Hip(0, seed=6)
    r, f = 3, 1
    even, odd, smp, err, tim, _ = filtered_target(scene, hip, 0, 4, 128, 0.02, r=r, f=f)
    full = NT.device_film(scene, hip, 0, 128)
    q = NT.queue(scene, 0)
    m = 2 + r   # (a sample reaches 2 pixels in each direction, the filter's window r more: a window of background averages to 0 in both halves)
    pad = np.pad(np.abs(full[..., :3]).sum(-1), m)
    dark = np.array([pad[8 * int(y):8 * int(y) + 8 + 2 * m, 8 * int(x):8 * int(x) + 8 + 2 * m].max() == 0.0 for x, y in q])
    print(f"{dark.sum()} of {len(q)} tiles see only background; samples per tile: {np.unique(smp, return_counts=True)}")
    assert dark.sum() >= 4 and (~dark).sum() >= 4
    assert (smp[dark] == 4).all() and (err[dark] == 0.0).all()
    assert (smp[~dark] > 4).any()
    assert tim.samples == int((64 * smp.astype(np.int64)).sum())
    assert (err[smp < 128] < 0.02).all()


def test_python_render_denoised_filtered(tmp_path):
    w, h, spp, lo, thr = 160, 96, 64, 8, 0.0
    scene, rt, _, fi = NT.load(scenes.cornell_box(w, h, spp), tmp_path)
    cfg = T.Config(str(tmp_path), "s.json", spp, 1, fi)
    hip = T.Hip(0, seed=9)
    with pytest.raises(ValueError):
        hip.render_denoised(scene, rt, cfg, error="filtered")
    with pytest.raises(ValueError):
        hip.render_denoised(scene, rt, cfg, threshold=0.1, error="denoised")
    with pytest.raises(ValueError):
        hip.render_noise_target(scene, rt, cfg, 0.1, error="")
    rt.clear()
    # far from any tile's error (threshold 0) the tile samples are decided the same way in every run: the result is the C call's
    smp, err = hip.render_denoised(scene, rt, cfg, threshold=thr, min_spp=lo, error="filtered")
    got = rt.get_renderf32().reshape(h, w, 4)
    even, odd, smp_c, err_c, _, out_c = filtered_target(scene, T.Hip(0, seed=9), 0, lo, spp, thr, with_out=True)
    assert (smp == smp_c).all() and (smp == spp).all()
    np.testing.assert_allclose(err, err_c, rtol=1e-3)
    D.assert_matches(got, even, odd, R_, F_, K_, "render_denoised(error='filtered') against the statement on the C call's films")
    D.assert_matches(out_c, even, odd, R_, F_, K_, "the C call's out_dev against the statement on its films")
    # a real threshold: it denoises
    rt.clear()
    smp, err = hip.render_denoised(scene, rt, cfg, threshold=0.15, min_spp=lo, error="filtered")
    den = rt.get_renderf32().reshape(h, w, 4)
    rt.clear()
    smp_n, _ = T.Hip(0, seed=9).render_noise_target(scene, rt, cfg, 0.15, min_spp=lo, error="filtered")
    noisy = rt.get_renderf32().reshape(h, w, 4)
    scene.release_device()
    ref = reference_image(scene, 4096, seed=1234)
    with np.errstate(all="ignore"):
        noisy_rgb = np.where(noisy[..., 3:] > 0, noisy[..., :3] / noisy[..., 3:], 0)
    e_noisy = float(np.sqrt(np.mean((noisy_rgb - ref) ** 2)))
    e_den = float(np.sqrt(np.mean((den[..., :3] - ref) ** 2)))
    print(f"threshold 0.15: mean n_t {smp.mean():.1f} / {smp_n.mean():.1f}, RMSE(even + odd) = {e_noisy:.5f}, RMSE(denoised) = {e_den:.5f}")
    assert e_den < e_noisy


def test_full_size_frame(tmp_path):
    w, h, lo, hi = 1920, 1080, 16, 256
    scene, *_ = NT.load(scenes.cornell_box(w, h, hi), tmp_path)
    hip = T.Hip(0, seed=3)
    even, odd, smp, err, tim, out = filtered_target(scene, hip, 0, lo, hi, 0.1, with_out=True)
    print(f"1920x1080: samples per tile {np.unique(smp, return_counts=True)}, {tim.render_ms:.1f} ms, {tim.launches} launches")
    assert np.isfinite(even).all() and np.isfinite(odd).all() and np.isfinite(out).all() and (out[..., 3] == 1.0).all()
    assert not np.isnan(err).any()
    assert all(lo <= n <= hi and (n & (n - 1)) == 0 for n in np.unique(smp))
    assert tim.samples == int((NT.pixels_in_image(scene, 0, NT.queue(scene, 0)) * smp.astype(np.int64)).sum())
    assert tim.launches == launches_of(smp, lo, True)
