"""What the tests of the noise-target calls' neighbour bound share (include/trayhip.h: tray_scene_set_noise_ratio): the numpy statement of the
rounds -- the set S that renders next as a naive fixed-point iteration over a dict of tiles, the level lists, the end state --, the checks of a
result (the ratio invariant, powers of two), the loader of the host emulation (tests/emu/emu_nbound.cpp) and one emulated call over it, and the
scene of the emulation and GPU tests. Test infrastructure only."""
import ctypes as C
import functools
import os
import types

import numpy as np

import _emu as E
import _emu_features as EF
import _noise_plan as NP

GUARD = EF.GUARD
NO_TILE = 0xffffffff
BOUND_REGIONS = ("lists", "lists_q", "map", "counts")
AROUND = [(dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0)]


# ---- the rule in numpy / plain Python

def levels_of(lo, hi):
    return int(np.log2(hi // lo)) + 1


def neighbours(tiles, t):
    """the tiles of the dict `tiles` among the eight around t"""
    return [(t[0] + dx, t[1] + dy) for dx, dy in AROUND if (t[0] + dx, t[1] + dy) in tiles]


def next_set(tiles, keep, ratio, max_spp):
    """The set that renders the next round. tiles: {(x, y): n_t} of the call's range; keep: the tiles rule (a) keeps. The least set S that holds
    `keep` and every tile t with n_t < max_spp that has a neighbour u with n_u' > ratio n_t, n_u' = 2 n_u if u is in S, else n_u: sweeps over all
    tiles until a sweep adds nothing."""
    S = set(keep)
    if not ratio:
        return S
    grew = True
    while grew:
        grew = False
        for t, n_t in tiles.items():
            if t in S or n_t >= max_spp:
                continue
            if any(tiles[u] * (2 if u in S else 1) > ratio * n_t for u in neighbours(tiles, t)):
                S.add(t)
                grew = True
    return S


def level_lists(queue, samples, flags, lo, levels):
    """per level that can render, the queue indices of the flagged tiles with samples == lo 2^l, in queue order"""
    samples, flags = np.asarray(samples), np.asarray(flags)
    return [np.flatnonzero((flags != 0) & (samples == (lo << l))).astype(np.uint32) for l in range(max(levels - 1, 0))]


def run_rounds(queue, noisy_after, lo, hi, ratio):
    """the rounds with errors from a table: tile i stays noisy while its n_t < noisy_after[i]; returns n_t per queue entry"""
    tiles = {(int(x), int(y)): lo for x, y in queue}
    index = {t: i for i, t in enumerate(tiles)}
    S = set(tiles)
    first = True
    while S:
        for t in S:
            tiles[t] = lo if first else 2 * tiles[t]
        first = False
        keep = {t for t in S if tiles[t] < noisy_after[index[t]] and tiles[t] < hi}
        S = next_set(tiles, keep, ratio, hi)
    return np.array([tiles[(int(x), int(y))] for x, y in queue], np.uint32)


def worst_ratio(queue, samples):
    """the largest n_t ratio over all pairs of neighbouring tiles of the queue"""
    tiles = {(int(x), int(y)): int(n) for (x, y), n in zip(queue, samples)}
    return max((max(n, tiles[u]) / min(n, tiles[u]) for t, n in tiles.items() for u in neighbours(tiles, t)), default=1.0)


def assert_result(queue, samples, lo, hi, ratio, what=""):
    samples = np.asarray(samples, np.int64)
    assert ((samples >= lo) & (samples <= hi) & ((samples & (samples - 1)) == 0)).all(), f"{what}: n_t is not a power of two in [{lo}, {hi}]: {samples.tolist()}"
    if ratio:
        assert worst_ratio(queue, samples) <= ratio, f"{what}: neighbouring tiles more than {ratio}x apart: {samples.tolist()}"


def filter_bounds(film):
    """What one camera sample can add to a pixel's weight, from the film's own filter table, per pixel offset o = (pixel - sample's pixel) in
    [-4, 4]^2 as (9, 9) arrays indexed [oy + 4, ox + 4]: (least, mean). RenderTarget::write (render_target.rs:77-165) gives a sample at image
    position c the weight table[iy, ix] at pixel p, with d = p + 0.5 - c per axis, i = min(floor(16 |d| inv_w), 15), and nothing where
    |d| inv_w > filter_w. A sample of pixel p - o has d in [o - 0.5, o + 0.5] per axis: `least` is the smallest weight over the table cells in
    that reach (0 if part of it lies past the filter), `mean` the average over the reach (the expectation for a position uniform in its pixel)."""
    tab = np.array(film.table[:], np.float64).reshape(16, 16)
    sub = 64   # the reach in steps of 1 / 64 pixel: cell borders lie at multiples of 1 / (16 inv_w) = 1 / 8

    def reach(o, inv, width, closed):
        d = np.abs(o + 0.5 - (np.arange(sub + 1) / sub if closed else (np.arange(sub) + 0.5) / sub))
        return np.minimum(np.floor(16 * d * inv).astype(int), 15), d * inv <= width

    least, mean = np.zeros((9, 9)), np.zeros((9, 9))
    for oy in range(-4, 5):
        for ox in range(-4, 5):
            (iy, my), (ix, mx) = reach(oy, film.inv_h, film.filter_h, True), reach(ox, film.inv_w, film.filter_w, True)
            least[oy + 4, ox + 4] = np.where(np.outer(my, mx), tab[np.ix_(iy, ix)], 0.0).min()
            (iy, my), (ix, mx) = reach(oy, film.inv_h, film.filter_h, False), reach(ox, film.inv_w, film.filter_w, False)
            mean[oy + 4, ox + 4] = np.where(np.outer(my, mx), tab[np.ix_(iy, ix)], 0.0).mean()
    return least, mean


def weight_floor(film, queue, samples, ratio, kind=0):
    """Per pixel of the w x h film, the lower bound on its weight w that `ratio` guarantees (test_gpu_nbound.py derives it): with n_t the samples
    of the pixel's own tile and K = filter_bounds(film)[kind], n_t (sum of K(o) over the pixels p - o of its own tile + ratio * sum of
    min(K(o), 0) over the pixels p - o of other tiles), pixels outside the image left out."""
    K = filter_bounds(film)[kind]
    w, h = film.width, film.height
    n_of = np.zeros((h, w))
    tile_id = np.full((h, w), -1)
    for i, ((x, y), n) in enumerate(zip(queue, samples)):
        n_of[8 * y:8 * y + 8, 8 * x:8 * x + 8], tile_id[8 * y:8 * y + 8, 8 * x:8 * x + 8] = n, i
    pad_id = np.pad(tile_id, 4, constant_values=-1)
    coeff = np.zeros((h, w))
    for oy in range(-4, 5):
        for ox in range(-4, 5):
            q = pad_id[4 - oy:4 - oy + h, 4 - ox:4 - ox + w]   # the tile of pixel p - o, -1 outside the image
            k = K[oy + 4, ox + 4]
            coeff += np.where(q == tile_id, k, np.where(q >= 0, ratio * min(k, 0.0), 0.0))
    return n_of * coeff


def oracle_film64(flat, queue, ranges, spp, seed):
    """The oracle's film of the samples [ranges[i][0], ranges[i][1]) of every pixel of tile queue[i] (a spp-sample frame), as _ranges.oracle_range
    builds it -- O.sample_radiance for the samples, O.film_patches for RenderTarget::write of each -- but summed in f64: at 64 samples per pixel an
    f32 sum over a pixel's ~1000 splats is itself some 1e-5 of the pixel's weight off, which is the bar the films are held to."""
    import _oracle as O
    from _emu import FILM_PATCH_R as r
    fs = flat.contents
    w, h = fs.film.width, fs.film.height
    pad = np.zeros((h + 2 * r, w + 2 * r, 4), np.float64)
    for tile, (begin, end) in zip(queue, ranges):
        if end <= begin:
            continue
        px, py = np.meshgrid(np.arange(8) + 8 * int(tile[0]), np.arange(8) + 8 * int(tile[1]))
        px, py = np.repeat(px.ravel(), end - begin), np.repeat(py.ravel(), end - begin)
        out = O.sample_radiance(flat, px, py, np.tile(np.arange(begin, end), 64), spp, seed=seed)
        patches = O.film_patches(fs.film, (int(tile[0]), int(tile[1])), np.concatenate([out[:, 3:5], out[:, 0:3]], 1), r)
        for (x, y), p in zip(np.floor(out[:, 3:5]).astype(int), patches):
            pad[y:y + 2 * r + 1, x:x + 2 * r + 1] += p
    return pad[r:r + h, r:r + w].copy()


# ---- the host emulation

@functools.lru_cache(None)
def lib():
    deps = EF._hip("nbound_kernels.h", "guide_kernels.h", "block_compact.h", "denoise_kernels.h", "dev_libm.h", "noise_kernels.h", "noise_plan.h")
    deps += [os.path.join(E.EMU_DIR, f) for f in ("emu_guide.cpp", "emu_denoise.cpp", "emu_noise.cpp", "noise_plan_record.h")] + E.denoise_plan_deps()
    h = C.CDLL(E.build("libtrayemu_nbound.so", "emu_nbound.cpp", deps))
    u32, ptr = C.c_uint32, C.c_void_p
    h.emu_nb_grid.restype, h.emu_nb_grid.argtypes = C.c_int, [ptr, u32, u32, u32, ptr]
    h.emu_nb_pull.restype, h.emu_nb_pull.argtypes = C.c_int, [ptr, u32, ptr, u32, u32, ptr, ptr, u32, u32]
    h.emu_nb_compact_level.restype, h.emu_nb_compact_level.argtypes = C.c_int, [ptr, ptr, ptr, u32, u32, ptr, ptr, ptr]
    h.emu_nbound_layout.argtypes = [u32, u32, u32, u32, ptr]
    h.emu_nbound_call_launches.restype, h.emu_nbound_call_launches.argtypes = u32, [C.c_int, C.c_int, u32, u32, u32, u32]
    h.emu_nbound_target.restype = C.c_int
    h.emu_nbound_target.argtypes = [ptr, u32, u32, u32, u32, u32, u32, C.c_float, ptr, ptr, ptr, u32, u32, C.c_float, ptr, ptr, u32, ptr, NP.RENDER_FN,
                                    NP.AFTER_READ_FN, ptr]
    return h


def bound_layout(n_tiles, gw, gh, levels):
    out = np.zeros(9, np.uint64)
    lib().emu_nbound_layout(n_tiles, gw, gh, levels, out.ctypes.data)
    return {k: (int(out[2 * i]), int(out[2 * i + 1])) for i, k in enumerate(BOUND_REGIONS)}, int(out[8])


def call_launches(filtered, with_out, rounds, groups, levels, per_render=1):
    return int(lib().emu_nbound_call_launches(int(filtered), int(with_out), rounds, groups, levels, per_render))


def grid_map(queue, gw, gh):
    """tr_nbound::grid in the emulation: the map as (gh, gw) words between guard words"""
    q = np.ascontiguousarray(queue, np.uint32)
    buf = np.full(gw * gh + 2 * GUARD, 0xA5A5A5A5, np.uint32)
    assert lib().emu_nb_grid(q.ctypes.data, len(q), gw, gh, buf[GUARD:].ctypes.data) == 0
    assert (buf[:GUARD] == 0xA5A5A5A5).all() and (buf[-GUARD:] == 0xA5A5A5A5).all(), "a write outside the map"
    return buf[GUARD:-GUARD].reshape(gh, gw).copy()


def pull_step(queue, grid, samples, active, ratio, max_spp):
    """one k_nb_pull launch; returns the flags after it"""
    q, m = np.ascontiguousarray(queue, np.uint32), np.ascontiguousarray(grid, np.uint32)
    s, a = np.ascontiguousarray(samples, np.uint32), np.array(active, np.uint32)
    assert lib().emu_nb_pull(q.ctypes.data, len(q), m.ctypes.data, m.shape[1], m.shape[0], s.ctypes.data, a.ctypes.data, ratio, max_spp) == 0
    return a


def compact_level(queue, active, samples, n_level):
    """one k_nb_compact_level launch; returns (out_xy, out_q, count) with 0xffffffff where the kernel wrote nothing"""
    n = len(queue)
    q, a, s = (np.ascontiguousarray(v, np.uint32) for v in (queue, active, samples))
    out_xy, out_q = np.full((max(n, 1), 2), NO_TILE, np.uint32), np.full(max(n, 1), NO_TILE, np.uint32)
    count = np.full(1, NO_TILE, np.uint32)
    assert lib().emu_nb_compact_level(q.ctypes.data, a.ctypes.data, s.ctypes.data, n_level, n, out_xy.ctypes.data, out_q.ctypes.data, count.ctypes.data) == 0
    return out_xy, out_q, int(count[0])


def target(queue, w, h, lo, hi, threshold, ratio, render, after_read=None, filt=None, with_out=False):
    """_noise_plan.noise_target with a neighbour bound (ratio 0: without one, through the entry point the bounded call takes): one emulated call
    over `queue`. render(B, sel, begin, end, film) adds samples [begin, end) of the tiles queue[sel] to film; after_read(B, n_words) is called when
    a round's kernels are done and the host has read its counts. B holds the buffers as numpy views, as noise_target's, and the bound's: lists
    (levels - 1, n, 2), lists_q (levels - 1, n), map (gh, gw) and bcounts ([0] listed blocks, [1 + l] level l's tiles). Returns (rc, launches, B)."""
    n = len(queue)
    levels, gw, gh = levels_of(lo, hi), (w + 7) // 8, (h + 7) // 8
    B = types.SimpleNamespace(queue=np.ascontiguousarray(queue, np.uint32).reshape(n, 2), even=np.zeros((h, w, 4), np.float32),
                              odd=np.zeros((h, w, 4), np.float32), out=np.full((h, w, 4), np.nan, np.float32) if with_out else None)
    (tl, tl_total), (fl, fl_total), (bl, bl_total) = NP.tile_layout(n), NP.filtered_layout(w, h), bound_layout(n, gw, gh, levels)
    tiles = np.full(tl_total + 2 * GUARD, 0xFF, np.uint8)
    scratch = np.full(fl_total + 2 * GUARD, 0xFF, np.uint8) if filt else None
    bound = np.full(bl_total + 2 * GUARD, 0xFF, np.uint8)
    view = lambda buf, region, dtype: buf[GUARD + region[0]:GUARD + region[0] + region[1]].view(dtype)
    B.list, B.list_q, B.active, B.samples = view(tiles, tl["list"], np.uint32).reshape(n, 2), *(view(tiles, tl[k], np.uint32) for k in ("list_q", "active", "samples"))
    B.err, B.counts = view(tiles, tl["err"], np.float32), view(tiles, tl["count"], np.uint32)
    rows = max(levels - 1, 1)
    B.lists, B.lists_q = view(bound, bl["lists"], np.uint32).reshape(rows, n, 2), view(bound, bl["lists_q"], np.uint32).reshape(rows, n)
    B.map, B.bcounts = view(bound, bl["map"], np.uint32).reshape(gh, gw), view(bound, bl["counts"], np.uint32)
    if filt:
        B.fa, B.fb = (view(scratch, fl[k], np.float32).reshape(h, w, 4) for k in ("fa", "fb"))
        B.flags, B.blocks = (view(scratch, fl[k], np.uint32) for k in ("flags", "list"))
        if not ratio:
            B.counts = view(scratch, fl["counts"], np.uint32)
    raised = []

    def guarded(fn):
        def call(*args):
            try:
                fn(*args)
                return 0
            except BaseException as e:   # (an exception does not cross a ctypes callback: stop the schedule, raise below)
                raised.append(e)
                return 1
        return call

    @guarded
    def on_render(list_ptr, n_list, begin, end, film_ptr):
        lists = {B.queue.ctypes.data: None, B.list.ctypes.data: B.list_q}
        lists.update({B.lists[l].ctypes.data: B.lists_q[l] for l in range(rows)})
        assert list_ptr in lists, "a tile list that is none of the call's"
        sel = np.arange(n_list) if lists[list_ptr] is None else lists[list_ptr][:n_list].copy()
        film = {B.even.ctypes.data: B.even, B.odd.ctypes.data: B.odd}[film_ptr]
        render(B, sel, begin, end, film)

    @guarded
    def on_read(counts_ptr, n_words):
        if after_read is not None:
            after_read(B, n_words)

    launches = C.c_uint32(0)
    r, f, k = filt or (0, 0, 0.0)
    rc = lib().emu_nbound_target(B.queue.ctypes.data, n, n, w, h, lo, hi, threshold, B.even.ctypes.data, B.odd.ctypes.data, tiles[GUARD:].ctypes.data, r, f, k,
                                 scratch[GUARD:].ctypes.data if filt else None, B.out.ctypes.data if with_out else None, ratio, bound[GUARD:].ctypes.data,
                                 NP.RENDER_FN(on_render), NP.AFTER_READ_FN(on_read), C.byref(launches))
    if raised:
        raise raised[0]
    for buf in (tiles, bound, scratch) if filt else (tiles, bound):
        assert (buf[:GUARD] == 0xFF).all() and (buf[-GUARD:] == 0xFF).all(), "a write outside the per-tile buffers, the bound's or the scratch buffer"
    return rc, launches.value, B
