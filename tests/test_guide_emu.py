"""The kernels of the filtered stopping rule (guide_kernels.h) in the host emulation, against the numpy statements of tests/_guide_ref.py.

tests/emu/emu_guide.cpp runs k_dn_filter_halves, k_guide_mark and k_guide_compact as SIMT fibers. Bars: each filtered half within 4 x the f32
statement's distance from the f64 one on that half, plus 1e-7 (_denoise_ref.bar's rule); (fa + fb) * 0.5 equal to the emulated k_dn_filter's
output bit for bit; with a block list, the listed blocks equal to the full run bit for bit and every other word untouched; the block list exactly
numpy's. Then the rounds of tray_render_noise_target_filtered_device on films of the oracle: the library's schedule (noise_plan.h) over the emulated
kernels, with a stand-in for the range launches, observed from Python whenever the host has read a round's counts: errors within 4 ulps of the
numpy metric of the emulated halves, flags and lists exact, n_t the numpy rule's at thresholds no tile's f64 error lies within 1e-3 relative of,
the final filter's output a tray_denoise_device call's. The raw rule's rounds (tray_render_noise_target_device) go through the same schedule. And
the property the rule rests on: at 32 samples at least 90 % of the tiles have a smaller filtered than raw error."""
import json
import os
import types

import numpy as np
import pytest

import tray_rust_amd as T
from tray_rust_amd import scenes
import _denoise_ref as D
import _emu_features as EF
import _guide_ref as G
import _noise_plan as NP
import _noise_ref as N
import _ranges as R
from _emu_features import SENTINEL, guide_halves as run_halves

F32 = np.float32


@pytest.fixture(scope="module")
def guide():
    return EF.guide_lib()


@pytest.fixture(scope="module")
def denoise():
    return EF.denoise_lib()


SIZES = [(67, 45), (160, 96)]
RF = [(1, 0), (3, 1), (7, 3), (10, 3)]


@pytest.mark.parametrize("r,f", RF, ids=[f"r{r}f{f}" for r, f in RF])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_halves_match_the_f64_statement_and_average_to_the_filter(guide, denoise, w, h, r, f):
    even, odd = D.random_films(w, h, seed=11 * w + h)
    fa, fb = run_halves(guide, even, odd, r, f, 0.45)
    G.assert_halves_match(fa, fb, even, odd, r, f, 0.45, f"{w}x{h} r={r} f={f}")
    assert (fa[..., 3] == 0).any() or (fb[..., 3] == 0).any() or f > 0   # (patch 0: an invalid pixel has no partner and no weight)
    out = EF.denoise(denoise, even, odd, r, f, 0.45)
    mean = ((fa[..., :3] + fb[..., :3]) * F32(0.5)).astype(F32)
    assert (mean.view(np.uint32) == out[..., :3].view(np.uint32)).all(), "(fa + fb) * 0.5 is not k_dn_filter's output to the bit"


@pytest.mark.parametrize("which", ["empty", "last-row-and-column", "all", "scattered", "unordered-with-one-outside"])
@pytest.mark.parametrize("w,h", SIZES, ids=[f"{w}x{h}" for w, h in SIZES])
def test_a_block_list_computes_the_listed_blocks_only(guide, w, h, which):
    assert (w, h) != SIZES[0] or (w % G.BW and h % G.BH)   # (the first size is no multiple of the block: its last row and column are partial)
    even, odd = D.random_films(w, h, seed=3 * w + h)
    r, f = 7, 3
    full = run_halves(guide, even, odd, r, f, 0.45)
    blocks = G.block_lists(w, h)[which]
    got = run_halves(guide, even, odd, r, f, 0.45, blocks=blocks)
    bx, by = G.blocks_of(w, h)
    mask = G.block_mask([b for b in blocks if b < bx * by], w, h)
    assert mask.sum() == (0 if which == "empty" else w * h if which == "all" else mask.sum())
    for g, want in zip(got, full):
        assert (g.view(np.uint32)[mask] == want.view(np.uint32)[mask]).all(), "a listed block differs from the full run"
        assert (g.view(np.uint32)[~mask] == SENTINEL).all(), "a pixel outside the listed blocks was written"


def run_block_list(guide, queue, active, w, h):
    """k_guide_mark over zeroed flags, then k_guide_compact: (list, count), the list between sentinel words"""
    bx, by = G.blocks_of(w, h)
    queue = np.ascontiguousarray(queue, np.uint32).reshape(-1, 2)
    flags = np.zeros(bx * by + 2, np.uint32)
    flags[0] = flags[-1] = SENTINEL
    act = None if active is None else np.ascontiguousarray(active, np.uint32)
    assert guide.emu_guide_mark(queue.ctypes.data, None if act is None else act.ctypes.data, len(queue), w, h, flags[1:].ctypes.data) == 0
    assert flags[0] == SENTINEL and flags[-1] == SENTINEL and np.isin(flags[1:-1], (0, 1)).all()
    out = np.full(bx * by + 2, SENTINEL, np.uint32)
    count = np.full(1, SENTINEL, np.uint32)
    assert guide.emu_guide_compact(flags[1:].ctypes.data, w, h, out[1:].ctypes.data, count.ctypes.data) == 0
    n = int(count[0])
    assert n <= bx * by and (out[1 + n:] == SENTINEL).all() and out[0] == SENTINEL, "a write outside the list"
    return out[1:1 + n].copy()


@pytest.mark.parametrize("w,h", SIZES + [(1920, 1080)], ids=[f"{w}x{h}" for w, h in SIZES + [(1920, 1080)]])
def test_block_lists_are_numpys(guide, w, h):
    queue = N.tiles_over(w, h)
    rng = np.random.default_rng(w)
    rng.shuffle(queue)   # (the library's queue is in Morton order: any order must do)
    n = len(queue)
    single = np.zeros(n, np.uint32); single[n // 2] = 1
    cases = {"none-given": None, "empty": np.zeros(n, np.uint32), "full": np.ones(n, np.uint32), "single": single,
             "sparse": (rng.random(n) < 0.02).astype(np.uint32), "half": (rng.random(n) < 0.5).astype(np.uint32) * rng.integers(1, 4, n).astype(np.uint32)}
    bx, by = G.blocks_of(w, h)
    for name, active in cases.items():
        got = run_block_list(guide, queue, active, w, h)
        want = G.block_list(queue, active, w, h)
        assert len(got) == len(want) and (got == want).all(), (name, got[:8], want[:8])
    assert len(run_block_list(guide, queue, None, w, h)) == bx * by and len(run_block_list(guide, queue, cases["empty"], w, h)) == 0
    assert len(run_block_list(guide, queue, single, w, h)) == 1
    # a tile outside the frame's blocks is passed over
    far = np.concatenate([queue[:3], np.array([[4 * bx, 0], [0, 2 * by]], np.uint32)])
    assert (run_block_list(guide, far, None, w, h) == G.block_list(queue[:3], None, w, h)).all()


# ---- the rounds on films of the oracle

W = H = 64
MIN_SPP, MAX_SPP = 8, 128
SEED = 7
R_, F_, K_ = 7, 3, 0.45


@pytest.fixture(scope="module")
def oracle_rounds(tmp_path_factory, built):
    """per scene: the queue and the oracle's film of every sample range a call may render, by (begin, end): each round's two halves alone"""
    out = {}
    for name in ("cornell_box", "smallpt"):
        d = str(tmp_path_factory.mktemp("guide_" + name))
        scenes.write_assets(d)
        p = os.path.join(d, "s.json")
        with open(p, "w") as fh:
            json.dump(getattr(scenes, name)(W, H, MAX_SPP), fh)
        scene, *_ = T.Scene.load_file(p)
        flat = scene.flatten(0)
        queue = R.tile_queue(W, H)
        ranges = {}
        lo, hi = 0, MIN_SPP
        while hi <= MAX_SPP:
            mid = lo + (hi - lo) // 2
            ranges.update({rng: R.oracle_range(flat, queue, rng, MAX_SPP, SEED)[0] for rng in ((lo, mid), (mid, hi))})
            lo, hi = hi, hi * 2
        out[name] = (queue, ranges)
    return out


def tile_mask(queue, sel):
    m = np.zeros((H, W), bool)
    for x, y in queue[sel]:
        m[8 * y:8 * y + 8, 8 * x:8 * x + 8] = True
    return m


def assert_halves_over(guide, B, blocks, sel, queue):
    """B.fa / B.fb equal the halves of B's films over the whole frame on the listed blocks, bit for bit, and the tiles queue[sel] lie inside those"""
    m, bm = tile_mask(queue, sel), G.block_mask(blocks, W, H)
    assert m[bm].sum() == m.sum(), "an active tile outside the listed blocks"
    whole = run_halves(guide, B.even, B.odd, R_, F_, K_)
    assert all((a.view(np.uint32)[bm] == b.view(np.uint32)[bm]).all() for a, b in ((B.fa, whole[0]), (B.fb, whole[1])))


def f64_tile_errors(B, tiles, filtered):
    """the numpy rule in f64: the tiles' errors on the f64 halves of B's films (the raw rule: on the films)"""
    fa64, fb64 = B.even, B.odd
    if filtered:
        A64, wA, B64, wB = G.halves(B.even, B.odd, R_, F_, K_, np.float64)
        fa64, fb64 = np.concatenate([A64, wA[..., None]], -1), np.concatenate([B64, wB[..., None]], -1)
    return np.array([G.tile_error(fa64, fb64, t, np.float64) for t in tiles])


def drive_rounds(guide, queue, ranges, threshold, filtered=True, with_out=False):
    """One tray_render_noise_target_filtered_device call (filtered False: tray_render_noise_target_device, the error that of the films themselves) in
    the emulation -- the library's schedule (noise_plan.h) over the emulated kernels --, every round checked against numpy when the host has read
    its counts. The render stand-in adds the oracle's range films inside the listed tiles (the splats across tile borders stay with the tile that
    took the sample only approximately so: the stand-in is exact in what the rule reads, the films as they stand). Returns n_t and the last error
    per tile, the f64 numpy rule's n_t (None if it kept other tiles in some round), every f64 error it compared with the threshold, the buffers."""
    n = len(queue)
    want_nt, want_active, err64_seen = np.zeros(n, np.uint32), np.ones(n, bool), []
    st = types.SimpleNamespace(sel=None, hi=0, blocks=None, agree=True, rounds=0)

    def render(B, sel, begin, end, film):
        m = tile_mask(queue, sel)
        film[m] += ranges[begin, end][m]
        st.sel, st.hi = sel, end

    def after_read(B, first, n_words):
        sel, hi, blocks = st.sel, st.hi, st.blocks
        st.blocks = B.blocks[:int(B.counts[1])].copy() if filtered else None   # the list the next round filters over
        if sel is None:   # nothing is rendered yet: the blocks of the whole queue, a read of one word
            assert filtered and (first, n_words) == (1, 1) and np.array_equal(st.blocks, G.block_list(queue, None, W, H))
            return
        assert (first, n_words) == (0, 2 if filtered else 1), "a round reads its counts in one copy"
        if filtered:
            assert_halves_over(guide, B, blocks, sel, queue)
        fe, fo = (B.fa, B.fb) if filtered else (B.even, B.odd)   # the two films the error is taken from
        N.assert_ulps(B.err[sel], np.array([G.tile_error(fe, fo, t) for t in queue[sel]], F32), 4, f"round to {hi}")
        with np.errstate(invalid="ignore"):
            assert (B.active[sel] == ((~(B.err[sel] < threshold)) & (hi < MAX_SPP)).astype(np.uint32)).all()
        assert (B.samples[sel] == hi).all()
        rest = np.setdiff1d(np.arange(n), sel)   # (the tiles that stopped earlier keep what they had)
        assert (B.active[rest] == 0).all() and (B.samples[rest] == want_nt[rest]).all()
        e64 = f64_tile_errors(B, queue[sel], filtered)
        err64_seen.append(e64)
        want_nt[sel] = hi
        want_active[np.setdiff1d(np.arange(n), sel[~(e64 < threshold) & (hi < MAX_SPP)])] = False
        # the next lists
        nxt = np.flatnonzero(B.active)
        assert int(B.counts[0]) == len(nxt) and (B.list_q[:len(nxt)] == nxt).all() and (B.list[:len(nxt)] == queue[nxt]).all()
        assert not filtered or np.array_equal(st.blocks, G.block_list(queue, B.active, W, H))
        st.agree = st.agree and np.array_equal(np.flatnonzero(want_active), nxt)   # (the f32 kernels and the f64 rule keep the same tiles)
        st.rounds += 1

    rc, launches, B = NP.noise_target(queue, W, H, MIN_SPP, MAX_SPP, threshold, render, after_read, filt=(R_, F_, K_) if filtered else None, with_out=with_out)
    assert rc == 0 and launches == NP.call_launches(filtered, with_out, st.rounds), (rc, launches, st.rounds)
    return B.samples.copy(), B.err.copy(), want_nt if st.agree else None, np.concatenate(err64_seen), B


# between 0.15 and 0.3, where the filtered tile errors of these films lie (median 0.07 ... 0.14, largest 0.14 ... 0.41 over the rounds); chosen so that
# the f64 statement's errors keep clear of them: the nearest lies 2.2e-3 relative away on cornell_box, 9e-3 on smallpt (asserted below as > 1e-3)
THRESHOLDS = {"cornell_box": [0.17, 0.22, 0.27], "smallpt": [0.17, 0.22, 0.27]}


@pytest.mark.parametrize("name", ["cornell_box", "smallpt"])
def test_rounds_on_oracle_films(guide, oracle_rounds, name):
    queue, ranges = oracle_rounds[name]
    counts = []
    for thr in THRESHOLDS[name]:
        assert 0.15 <= thr <= 0.3
        samples, err, want_nt, e64, B = drive_rounds(guide, queue, ranges, F32(thr), with_out=thr == THRESHOLDS[name][-1])
        if B.out is not None:   # the final filter of the films as the call leaves them: a tray_denoise_device call's output
            assert (B.out.view(np.uint32) == EF.denoise(EF.denoise_lib(), B.even, B.odd, R_, F_, K_).view(np.uint32)).all()
        rel = np.abs(e64[np.isfinite(e64)] - float(F32(thr))) / float(F32(thr))
        assert rel.min() > 1e-3, f"{name}: a tile's f64 error lies within 1e-3 relative of the threshold {thr}: choose another"
        assert want_nt is not None and (samples == want_nt).all(), "n_t is not the numpy rule's"
        assert ((samples >= MIN_SPP) & (samples <= MAX_SPP) & (samples & (samples - 1) == 0)).all()
        counts.append(float(samples.mean()))
        print(f"{name} threshold {thr}: mean n_t {samples.mean():.1f}, tiles at max_spp {int((samples == MAX_SPP).sum())} of {len(samples)}")
    assert counts[0] >= counts[1] >= counts[2] and counts[0] > counts[2], counts   # a tighter threshold takes more samples


# the raw rule over the same films: its tile errors are larger (median 0.32 ... 0.40, largest 0.64 ... 0.70 over the rounds). From a scan of 0.20 ... 0.65 in
# steps of 0.01 with the f64 statement alone: the nearest f64 error lies 6.4e-3, 1.9e-2, 2.4e-2 relative away on cornell_box, 7.5e-3, 6.9e-3, 1.8e-2 on smallpt
RAW_THRESHOLDS = {"cornell_box": [0.29, 0.41, 0.55], "smallpt": [0.22, 0.31, 0.48]}


@pytest.mark.parametrize("name", ["cornell_box", "smallpt"])
def test_rounds_of_the_raw_rule_on_oracle_films(guide, oracle_rounds, name):
    """tray_render_noise_target_device through the same schedule: no block lists, one count word per round, the error of the films themselves"""
    queue, ranges = oracle_rounds[name]
    counts = []
    for thr in RAW_THRESHOLDS[name]:
        samples, err, want_nt, e64, _ = drive_rounds(guide, queue, ranges, F32(thr), filtered=False)
        rel = np.abs(e64[np.isfinite(e64)] - float(F32(thr))) / float(F32(thr))
        assert rel.min() > 1e-3, f"{name}: a tile's f64 error lies within 1e-3 relative of the threshold {thr}: choose another"
        assert want_nt is not None and (samples == want_nt).all(), "n_t is not the numpy rule's"
        assert ((samples >= MIN_SPP) & (samples <= MAX_SPP) & (samples & (samples - 1) == 0)).all()
        counts.append(float(samples.mean()))
        print(f"{name} threshold {thr}: mean n_t {samples.mean():.1f}, tiles at max_spp {int((samples == MAX_SPP).sum())} of {len(samples)}")
    assert counts[0] > counts[1] > counts[2] > MIN_SPP, counts


@pytest.mark.parametrize("name", ["cornell_box", "smallpt"])
def test_the_filtered_error_is_below_the_raw_one_at_32_samples(guide, oracle_rounds, name):
    """the property the rule rests on: where the filter helps, the difference of the filtered halves is smaller than that of the films"""
    queue, ranges = oracle_rounds[name]
    even, odd = np.zeros((H, W, 4), F32), np.zeros((H, W, 4), F32)
    for i, ((begin, end), film) in enumerate(ranges.items()):   # (in the fixture's order: a round's first half, for even, then its second, for odd)
        if end <= 32:
            (odd if i % 2 else even)[...] += film
    fa, fb = run_halves(guide, even, odd, R_, F_, K_)
    raw = np.array([N.numpy_tile_error(even, odd, t) for t in queue])
    filt = np.array([G.tile_error(fa, fb, t) for t in queue])
    share = float((filt < raw).mean())
    print(f"{name} at n_t = 32: raw tile error median / max {np.median(raw):.3f} / {raw.max():.3f}, filtered {np.median(filt):.3f} / {filt.max():.3f}, "
          f"tiles with filtered < raw {share:.3f}")
    assert share >= 0.9
