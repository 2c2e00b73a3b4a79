"""tray_rust_amd/csrc/hip/noise_plan.h -- the rules, layouts and schedule of the two noise-target calls -- through the exports of the guide kernels'
emulation library (tests/emu/emu_guide.cpp, noise_plan_record.h): the layouts as {region: (offset, bytes)}, the schedule as a recording Ops lists
it for scripted count reads, and one emulated call over the real kernels with the test's render stand-in. Test infrastructure only."""
import ctypes as C
import functools
import types

import numpy as np

import _emu_features as EF

GUARD = EF.GUARD
GROUPS = ("render", "block_list", "halves", "error", "compact", "read", "final_filter")   # nt_record::Group
BUFFERS = ("null", "queue", "even", "odd", "tiles", "scratch", "out", "unknown")          # nt_record::Buffer
ROW = 12
# a group's arguments in the order noise_plan_record.h notes them; those in POINTERS are (buffer, offset) words
ARGS = {"render": ("list", "n", "begin", "end", "film"),
        "block_list": ("queue", "active", "n", "flags", "list", "count"),
        "halves": ("even", "odd", "records", "radius", "patch", "blocks", "n_blocks", "fa", "fb"),
        "error": ("fe", "fo", "list", "list_q", "n", "taken", "max_spp", "err", "active", "samples"),
        "compact": ("queue", "active", "n", "list", "list_q", "count"),
        "read": ("counts", "n_words"),
        "final_filter": ("even", "odd", "radius", "patch", "out", "records")}
POINTERS = {"list", "film", "queue", "active", "flags", "count", "even", "odd", "records", "blocks", "fa", "fb", "fe", "fo", "list_q", "err", "samples",
            "counts", "out"}
TILE_REGIONS = ("list", "list_q", "active", "samples", "err", "count")
FILTERED_REGIONS = ("records", "fa", "fb", "flags", "list", "counts")
RENDER_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p)
AFTER_READ_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_uint32)


@functools.lru_cache(None)
def lib():
    h = EF.guide_lib()
    u32, u64, ptr = C.c_uint32, C.c_uint64, C.c_void_p
    h.emu_noise_plan_constants.argtypes = [ptr]
    h.emu_noise_plan_call_launches.restype, h.emu_noise_plan_call_launches.argtypes = u32, [C.c_int, C.c_int, u32, u32]
    h.emu_noise_plan_tile_layout.argtypes = [u32, ptr]
    h.emu_noise_plan_filtered_layout.argtypes = [u32, u32, ptr]
    h.emu_noise_plan_scratch_bytes.restype, h.emu_noise_plan_scratch_bytes.argtypes = u64, [u32, u32]
    h.emu_noise_plan_frame_blocks.restype, h.emu_noise_plan_frame_blocks.argtypes = u32, [u32, u32]
    h.emu_noise_plan_rules.restype = C.c_int
    h.emu_noise_plan_rules.argtypes = [C.c_int, C.c_int, u32, C.c_int, u32, u32, u32, u32, C.c_float, ptr, ptr, u32, u32, C.c_float, ptr, ptr, ptr, ptr, ptr, u32]
    h.emu_noise_plan_record.restype = u32
    h.emu_noise_plan_record.argtypes = [C.c_int, C.c_int, u32, u32, u32, u32, u32, u32, u32, ptr, u32, ptr, u32, ptr, ptr]
    h.emu_noise_target.restype = C.c_int
    h.emu_noise_target.argtypes = [ptr, u32, u32, u32, u32, u32, u32, C.c_float, ptr, ptr, ptr, u32, u32, C.c_float, ptr, ptr, RENDER_FN, AFTER_READ_FN, ptr]
    return h


def constants():
    names = ("block_list", "error", "compact", "halves_of_no_block", "halves", "final_filter", "round_raw", "round_filtered")
    out = np.zeros(len(names), np.uint32)
    lib().emu_noise_plan_constants(out.ctypes.data)
    return dict(zip(names, (int(v) for v in out)))


def call_launches(filtered, with_out, rounds, per_render=1):
    return int(lib().emu_noise_plan_call_launches(int(filtered), int(with_out), rounds, per_render))


def _layout(export, names, *args):
    out = np.zeros(13, np.uint64)
    export(*args, out.ctypes.data)
    return {k: (int(out[2 * i]), int(out[2 * i + 1])) for i, k in enumerate(names)}, int(out[12])


def tile_layout(n_tiles):
    """({region: (offset, bytes)} in the order of the plan's struct, total)"""
    return _layout(lib().emu_noise_plan_tile_layout, TILE_REGIONS, n_tiles)


def filtered_layout(w, h):
    return _layout(lib().emu_noise_plan_filtered_layout, FILTERED_REGIONS, w, h)


def rules(filtered=False, scene=True, sampler=0, broken=False, w=64, h=48, lo=8, hi=64, thr=0.05, even=0x1000, odd=0x2000, r=7, f=3, k=0.45, out=0,
          scratch=0x3000, sm=0x4000, er=0x5000):
    """(return code, message) of a call's rules; the buffers are addresses that nothing follows"""
    msg = C.create_string_buffer(256)
    rc = lib().emu_noise_plan_rules(int(filtered), int(scene), sampler, int(broken), w, h, lo, hi, thr, even, odd, r, f, k, out, scratch, sm, er, msg, 256)
    return rc, msg.value.decode()


def record(filtered, with_out, w, h, n_tiles, tile_count, lo, hi, script, per_render=1):
    """the schedule of one call with its count reads answered from `script` (words, in the order they are read; zeros once used up):
    ([(group, {argument: value})], return code, launches). A pointer reads "queue", "even", "null", "tiles.samples", "scratch.counts+4"."""
    regions = {"tiles": tile_layout(n_tiles)[0], "scratch": filtered_layout(w, h)[0]}
    script = np.ascontiguousarray(script, np.uint32)
    cap = 16 * (int(np.log2(hi // lo)) + 2) if lo and hi >= lo else 64
    rows = np.zeros((cap, ROW), np.uint64)
    rc, launches = C.c_int(0), C.c_uint32(0)
    n = lib().emu_noise_plan_record(int(filtered), int(with_out), w, h, n_tiles, tile_count, lo, hi, per_render, script.ctypes.data, len(script),
                                    rows.ctypes.data, cap, C.byref(rc), C.byref(launches))
    assert n <= cap, n

    def where(word):
        buf, off = BUFFERS[word >> 56], word & ((1 << 56) - 1)
        if buf not in regions:
            return buf
        name, start = next((k, o) for k, (o, b) in regions[buf].items() if o <= off < o + b)
        return f"{buf}.{name}" + (f"+{off - start}" if off != start else "")

    events = []
    for row in rows[:n]:
        group = GROUPS[int(row[0])]
        events.append((group, {a: where(int(v)) if a in POINTERS else int(v) for a, v in zip(ARGS[group], row[1:])}))
    return events, rc.value, launches.value


def noise_target(queue, w, h, lo, hi, threshold, render, after_read=None, filt=None, with_out=False):
    """One emulated noise-target call over `queue`: the plan's schedule over the emulated kernels, the raw rule or, with filt = (radius, patch, k), the
    filtered one. render(B, sel, begin, end, film) is the stand-in for a range launch: it adds samples [begin, end) of the tiles queue[sel] to film
    (B.even or B.odd); after_read(B, first, n_words) is called when a round's kernels are done and the host has read counts[first, first + n_words).
    B holds the call's buffers as numpy views: queue, even, odd, out, the per-tile regions list (n, 2), list_q, active, samples, err, and the counts the
    rule reads; for the filtered rule fa, fb, flags and blocks too. Everything the kernels write lies between guard bytes and starts as 0xFF bytes
    (NaN as f32). An exception in a stand-in stops the schedule and is raised again here. Returns (return code, launches, B)."""
    n = len(queue)
    B = types.SimpleNamespace(queue=np.ascontiguousarray(queue, np.uint32).reshape(n, 2), even=np.zeros((h, w, 4), np.float32),
                              odd=np.zeros((h, w, 4), np.float32), out=np.full((h, w, 4), np.nan, np.float32) if with_out else None)
    (tl, tl_total), (fl, fl_total) = tile_layout(n), filtered_layout(w, h)
    tiles = np.full(tl_total + 2 * GUARD, 0xFF, np.uint8)
    scratch = np.full(fl_total + 2 * GUARD, 0xFF, np.uint8) if filt else None
    view = lambda buf, region, dtype: buf[GUARD + region[0]:GUARD + region[0] + region[1]].view(dtype)
    B.list, B.list_q, B.active, B.samples = view(tiles, tl["list"], np.uint32).reshape(n, 2), *(view(tiles, tl[k], np.uint32) for k in ("list_q", "active", "samples"))
    B.err, B.counts = view(tiles, tl["err"], np.float32), view(tiles, tl["count"], np.uint32)
    if filt:
        B.fa, B.fb = (view(scratch, fl[k], np.float32).reshape(h, w, 4) for k in ("fa", "fb"))
        B.flags, B.blocks, B.counts = (view(scratch, fl[k], np.uint32) for k in ("flags", "list", "counts"))
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
        if list_ptr == B.queue.ctypes.data:
            sel = np.arange(n_list)
        else:
            assert list_ptr == B.list.ctypes.data, "a tile list that is neither the queue nor the compacted list"
            sel = B.list_q[:n_list].copy()
            assert (B.list[:n_list] == B.queue[sel]).all()
        film = {B.even.ctypes.data: B.even, B.odd.ctypes.data: B.odd}[film_ptr]
        render(B, sel, begin, end, film)

    @guarded
    def on_read(counts_ptr, n_words):
        if after_read is not None:
            after_read(B, (counts_ptr - B.counts.ctypes.data) // 4, n_words)

    launches = C.c_uint32(0)
    r, f, k = filt or (0, 0, 0.0)
    rc = lib().emu_noise_target(B.queue.ctypes.data, n, n, w, h, lo, hi, threshold, B.even.ctypes.data, B.odd.ctypes.data, tiles[GUARD:].ctypes.data, r, f, k,
                                scratch[GUARD:].ctypes.data if filt else None, B.out.ctypes.data if with_out else None, RENDER_FN(on_render),
                                AFTER_READ_FN(on_read), C.byref(launches))
    if raised:
        raise raised[0]
    for buf in (tiles, scratch) if filt else (tiles,):
        assert (buf[:GUARD] == 0xFF).all() and (buf[-GUARD:] == 0xFF).all(), "a write outside the per-tile buffers or the scratch buffer"
    return rc, launches.value, B
