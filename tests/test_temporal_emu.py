"""tray_denoise_temporal_device's kernels (k_dn_prepare of denoise_kernels.h, k_tdn_pass of temporal_kernels.h) in the host emulation, against the
numpy statement of the temporal filter (tests/_temporal_ref.py, which restates include/trayhip.h in float32 and float64).

tests/emu/emu_temporal.cpp runs the 3 (N + 1) launches of a call as SIMT fibers: the LDS staging of each pass's frame, the two barriers per
offset and the sums carried from pass to pass in the scratch buffer execute as on the device. The bar of every comparison is
_temporal_ref.bar: the kernels may differ from the f64 statement by 4 x what the f32 numpy statement differs from it on the same input, plus
1e-7. Then: one frame gives the single-frame filter's bits, a neighbour without a valid pixel changes nothing, the scratch size, a constant
colour, and that the filter denoises three frames of the oracle's moving_box better than the single-frame filter does: at 64 x 64 and 32 spp the
f64 statement gives RMSE 0.01119 (temporal) / 0.01404 (spatial) / 0.02185 (noisy) against a 2048-spp oracle render of the centre frame."""
import json
import os

import numpy as np
import pytest

import tray_rust_amd as T
from tray_rust_amd import scenes
import _emu_features as EF
import _oracle as O
import _denoise_ref as D
import _ranges as R
import _temporal_ref as TR
from _denoise_ref import rgb, rmse
from _temporal_ref import run

F32 = np.float32


@pytest.fixture(scope="module")
def emu():
    return TR.temporal_lib()


SIZES = [(5, 3), (20, 12), (67, 45)]   # smaller than a window; not multiples of the 32 x 16 tile
RTF = [(1, 1, 0), (3, 2, 1), (7, 3, 3), (10, 7, 3)]
RF = [(1, 0), (3, 1), (7, 3), (10, 3)]   # test_denoise_emu.RF


@pytest.mark.parametrize("n", [1, 2])
@pytest.mark.parametrize("r,rt,f", RTF, ids=[f"r{r}t{rt}f{f}" for r, rt, f in RTF])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_emulated_kernels_match_the_f64_statement(emu, w, h, r, rt, f, n):
    frames = TR.random_frames(w, h, n + 1, seed=11 * w + h)
    for even, odd in frames:
        valid = D.resolve(even, odd)[0]
        assert (~valid).any() and valid.any()
    out = run(emu, frames, r, rt, f, 0.45)
    TR.assert_matches(out, frames, r, rt, f, 0.45, f"{w}x{h} r={r} rt={rt} f={f} N={n}")
    assert len(TR.range_violations(out[..., :3], frames, r, rt)) == 0


@pytest.mark.parametrize("r,f", RF, ids=[f"r{r}f{f}" for r, f in RF])
def test_one_frame_gives_the_single_frame_filters_bits(emu, r, f):
    spatial = EF.denoise_lib()
    for w, h in SIZES:
        even, odd = D.random_films(w, h, seed=11 * w + h)
        want = EF.denoise(spatial, even, odd, r, f, 0.45)
        got = run(emu, [(even, odd)], r, min(r, 3), f, 0.45)
        assert (got.view(np.uint32) == want.view(np.uint32)).all(), (w, h, int((got.view(np.uint32) != want.view(np.uint32)).sum()))
    # ... and the numpy statement of one frame is _denoise_ref's, operation for operation
    assert (TR.temporal([(even, odd)], r, 1, f, 0.45, F32).view(np.uint32) == D.denoise(even, odd, r, f, 0.45, F32).view(np.uint32)).all()


@pytest.mark.parametrize("kind", ["zero-weight", "nan", "negative-weight"])
def test_a_neighbour_without_a_valid_pixel_changes_nothing(emu, kind):
    w, h, (r, rt, f) = 41, 23, (7, 3, 3)
    centre, other = TR.random_frames(w, h, 2, seed=3)
    dead = np.ones((h, w, 4), F32)
    if kind == "zero-weight":
        dead[..., 3] = 0.0
    elif kind == "nan":
        dead[:] = np.nan
    else:
        dead[..., 3] = -2.0
    dead = (dead, dead.copy())
    alone = run(emu, [centre], r, rt, f, 0.45)
    assert (run(emu, [centre, dead], r, rt, f, 0.45).view(np.uint32) == alone.view(np.uint32)).all()
    # among valid neighbours, first and last: the bits of the call without it
    want = run(emu, [centre, other], r, rt, f, 0.45)
    assert (want.view(np.uint32) != alone.view(np.uint32)).any()
    for frames in ([centre, dead, other], [centre, other, dead]):
        got = run(emu, frames, r, rt, f, 0.45)
        assert (got.view(np.uint32) == want.view(np.uint32)).all()


def test_scratch_bytes_do_not_depend_on_the_neighbours(emu):
    assert emu.emu_temporal_scratch_bytes(0, 5) == 0 and emu.emu_temporal_scratch_bytes(5, 0) == 0
    assert emu.emu_temporal_scratch_bytes(67, 45) == 67 * 45 * 128
    # (run() keeps guard words around the output and a scratch buffer of exactly that size, with N = 0, 1 and 3)
    frames = TR.random_frames(33, 17, 4, seed=9)
    for n in (0, 1, 3):
        run(emu, frames[:n + 1], 3, 2, 1, 0.45)


def test_a_constant_colour_stays(emu):
    """one colour under arbitrary positive weights in every film of every frame: every weight is 1, the output is the colour within the range
    bound of all frames' offsets"""
    rng = np.random.default_rng(4)
    h, w = 30, 50
    colour = np.array([0.8, 0.25, 0.6], F32)
    frames = []
    for _ in range(3):
        pair = []
        for _ in range(2):
            wgt = rng.uniform(0.1, 50.0, (h, w, 1)).astype(F32)
            pair.append(np.concatenate([colour * wgt, wgt], -1).astype(F32))
        frames.append(tuple(pair))
    for r, rt, f in [(1, 1, 0), (7, 3, 3), (10, 7, 3)]:
        out = run(emu, frames, r, rt, f, 0.45)
        assert len(TR.range_violations(out[..., :3], frames, r, rt)) == 0
        assert np.abs(out[..., :3] - colour).max() <= (2 * TR.offsets(2, r, rt) + 4) * 2.0 ** -24 * 0.8 + 2.0 ** -23   # (+ the rounding of rgb w / w)


# ---- it denoises: films of the oracle

W = H = 64
SPP, SPLIT, REF_SPP = 32, 16, 2048
FRAMES, CENTRE = 48, 24


def test_it_denoises_a_moving_sequence_better_than_one_frame_alone(emu, tmp_path, built):
    """moving_box(frames=48), frames 23, 24, 25 at 32 spp, every half film of a seed of its own; RMSE against 2048 spp of frame 24"""
    scenes.write_assets(str(tmp_path))
    p = os.path.join(str(tmp_path), "s.json")
    with open(p, "w") as fh:
        json.dump(scenes.moving_box(W, H, SPP, frames=FRAMES), fh)
    scene, *_ = T.Scene.load_file(p)
    queue = R.tile_queue(W, H)
    pairs = {}
    for j, frame in enumerate((CENTRE, CENTRE - 1, CENTRE + 1)):
        flat = scene.flatten(frame)
        pairs[frame] = tuple(R.oracle_range(flat, queue, rng, SPP, 7 + 10 * j + i)[0] for i, rng in enumerate(((0, SPLIT), (SPLIT, SPP))))
    ref = rgb(O.render_tiles(scene.flatten(CENTRE), REF_SPP, seed=1234)[0])
    frames = [pairs[CENTRE], pairs[CENTRE - 1], pairs[CENTRE + 1]]   # the neighbours in ascending frame order
    r, rt, f, k = 7, 3, 3, 0.45
    out = run(emu, frames, r, rt, f, k)
    TR.assert_matches(out, frames, r, rt, f, k, "moving_box oracle films")
    spatial = run(emu, frames[:1], r, rt, f, k)
    noisy, one, three = rmse(rgb(frames[0][0] + frames[0][1]), ref), rmse(spatial[..., :3], ref), rmse(out[..., :3], ref)
    print(f"moving_box {W}x{H} {SPP} spp, frames 23 - 25: RMSE(noisy) = {noisy:.5f}, RMSE(spatial) = {one:.5f}, RMSE(temporal) = {three:.5f}")
    assert three < one < noisy
