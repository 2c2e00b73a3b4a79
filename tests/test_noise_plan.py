"""The one copy of the noise-target calls' rules, layouts and schedule (tray_rust_amd/csrc/hip/noise_plan.h), which libtrayhip.so and the host
emulation both run, reached through the exports of tests/emu/noise_plan_record.h (tests/_noise_plan.py): the regions of the per-tile buffers and
of the filtered rule's scratch are aligned, disjoint and end at the total, and the totals are the expressions the library used before the plan
existed; a recording Ops lists the schedule's launch groups with their arguments for scripted count reads; both TRAY_E_DEVICE refusals; every rule
by return code, and the first refusal in the calls' order. No GPU."""
import numpy as np
import pytest

import _noise_plan as NP

INVALID, UNSUPPORTED, DEVICE = -1, -4, -5   # include/trayhip.h


# ---- layouts

@pytest.mark.parametrize("n", [1, 48, 400_000_000], ids=["1", "48", "4e8-needs-64-bits"])
def test_tile_layout(n):
    regions, total = NP.tile_layout(n)
    assert list(regions) == ["list", "list_q", "active", "samples", "err", "count"]
    assert total == n * (8 + 4 * 4) + 4   # n (x, y) pairs and four words per tile, one count word
    assert n < 10 ** 8 or total > 2 ** 32
    end = 0
    for name, (off, size) in regions.items():
        assert off == end and size == (8 * n if name == "list" else 4 if name == "count" else 4 * n), name   # packed: disjoint, in rising order
        assert off % (8 if name == "list" else 4) == 0, name
        end = off + size
    assert end == total


@pytest.mark.parametrize("w,h", [(1, 1), (33, 17), (64, 48), (65535, 65535)], ids=["1x1", "33x17", "64x48", "65535x65535-needs-64-bits"])
def test_filtered_layout(w, h):
    regions, total = NP.filtered_layout(w, h)
    assert list(regions) == ["records", "fa", "fb", "flags", "list", "counts"]
    blocks = ((w + 31) // 32) * ((h + 15) // 16)
    assert NP.lib().emu_noise_plan_frame_blocks(w, h) == blocks
    # the filter's 48 bytes per pixel, fa and fb, a flag and a list word per block, four count words
    assert total == w * h * 48 + w * h * 32 + blocks * 8 + 16 == NP.lib().emu_noise_plan_scratch_bytes(w, h)
    assert w < 65535 or total > 2 ** 32
    sizes = {"records": 48 * w * h, "fa": 16 * w * h, "fb": 16 * w * h, "flags": 4 * blocks, "list": 4 * blocks, "counts": 16}
    end = 0
    for name, (off, size) in regions.items():
        assert off == end and size == sizes[name], name
        assert off % (16 if name in ("records", "fa", "fb") else 4) == 0, name   # the films and the records are read as float4
        end = off + size
    assert end == total


def test_scratch_bytes_of_an_empty_frame():
    assert NP.lib().emu_noise_plan_scratch_bytes(0, 48) == 0 and NP.lib().emu_noise_plan_scratch_bytes(64, 0) == 0


# ---- the schedule

W, H, N_TILES = 64, 48, 48
BLOCKS = 6
T, S = "tiles.", "scratch."


def expected(filtered, with_out, tile_count, lo, hi, actives, blocks=()):
    """the launch groups of a call whose reads answer actives[r] tiles (and blocks[r + 1] blocks, blocks[0] before round 0) after round r, written out"""
    counts = S + "counts" if filtered else T + "count"
    ev = []
    if filtered:
        ev += [("block_list", dict(queue="queue", active="null", n=tile_count, flags=S + "flags", list=S + "list", count=S + "counts+4")),
               ("read", dict(counts=S + "counts+4", n_words=1))]
    n, begin, end = tile_count, 0, lo
    for r, left in enumerate(actives):
        mid = (begin + end) // 2
        tiles, tiles_q = ("queue", "null") if r == 0 else (T + "list", T + "list_q")
        ev += [("render", dict(list=tiles, n=n, begin=begin, end=mid, film="even")), ("render", dict(list=tiles, n=n, begin=mid, end=end, film="odd"))]
        if filtered:
            ev += [("halves", dict(even="even", odd="odd", records=S + "records", radius=7, patch=3, blocks=S + "list", n_blocks=blocks[r], fa=S + "fa", fb=S + "fb"))]
        fe, fo = (S + "fa", S + "fb") if filtered else ("even", "odd")
        ev += [("error", dict(fe=fe, fo=fo, list=tiles, list_q=tiles_q, n=n, taken=end, max_spp=hi, err=T + "err", active=T + "active", samples=T + "samples")),
               ("compact", dict(queue="queue", active=T + "active", n=tile_count, list=T + "list", list_q=T + "list_q", count=counts))]
        if filtered:
            ev += [("block_list", dict(queue="queue", active=T + "active", n=tile_count, flags=S + "flags", list=S + "list", count=S + "counts+4"))]
        ev += [("read", dict(counts=counts, n_words=2 if filtered else 1))]
        n, begin, end = left, end, 2 * end
    if filtered and with_out:
        ev += [("final_filter", dict(even="even", odd="odd", radius=7, patch=3, out="out", records=S + "records"))]
    return ev


def script(filtered, actives, blocks):
    return list(actives) if not filtered else [blocks[0]] + [w for pair in zip(actives, blocks[1:]) for w in pair]


def launches_written_out(filtered, with_out, rounds):
    """mark and compact of the first block list; per round two renders, [prepare's two, the halves,] error, compact [, mark, compact]; the filter's three"""
    return (2 if filtered else 0) + rounds * (2 + (3 if filtered else 0) + 2 + (2 if filtered else 0)) + (3 if filtered and with_out else 0)


SCRIPTS = {   # (min_spp, max_spp, active tiles after each round, listed blocks before round 0 and after each round)
    "48-10-3-0": (8, 64, [10, 3, 0], [6, 4, 2, 0]),
    "never-empty-ends-at-max-spp": (8, 64, [48, 40, 40, 7], [6, 6, 6, 6, 3]),   # (the device sets no flag at max_spp; the schedule ends there whatever it reads)
    "min-equals-max": (16, 16, [0], [6, 0]),
    "one-tile-left-for-many-rounds": (2, 64, [1, 1, 1, 1, 0], [6, 1, 1, 1, 1, 0]),
}


@pytest.mark.parametrize("name", SCRIPTS)
@pytest.mark.parametrize("with_out", [False, True], ids=["no-out", "out"])
@pytest.mark.parametrize("filtered", [False, True], ids=["raw", "filtered"])
def test_schedule(filtered, with_out, name):
    lo, hi, actives, blocks = SCRIPTS[name]
    events, rc, launches = NP.record(filtered, with_out, W, H, N_TILES, N_TILES, lo, hi, script(filtered, actives, blocks))
    assert rc == 0
    want = expected(filtered, with_out, N_TILES, lo, hi, actives, blocks)
    assert events == want, next((i, a, b) for i, (a, b) in enumerate(zip(events + [None], want + [None])) if a != b)
    rounds = len(actives)
    assert sum(g == "read" for g, _ in events) == rounds + (1 if filtered else 0)   # one synchronisation per round, and the first block list's
    assert launches == launches_written_out(filtered, with_out, rounds) == NP.call_launches(filtered, with_out, rounds)
    # the rounds end with the first empty list, or at max_spp
    assert events[-1 - (1 if filtered and with_out else 0)][0] == "read" and (actives[-1] == 0 or lo << (rounds - 1) == hi)


def test_the_raw_rule_by_hand():
    """48 -> 10 -> 0 over tiles [0, 48) of a scene of 60, min_spp 4: every group and argument written out"""
    events, rc, launches = NP.record(False, False, W, H, 60, 48, 4, 64, [10, 0])
    tiles = dict(err="tiles.err", active="tiles.active", samples="tiles.samples")
    into = dict(queue="queue", active="tiles.active", n=48, list="tiles.list", list_q="tiles.list_q", count="tiles.count")
    assert rc == 0 and launches == 8 and events == [
        ("render", dict(list="queue", n=48, begin=0, end=2, film="even")), ("render", dict(list="queue", n=48, begin=2, end=4, film="odd")),
        ("error", dict(fe="even", fo="odd", list="queue", list_q="null", n=48, taken=4, max_spp=64, **tiles)), ("compact", into),
        ("read", dict(counts="tiles.count", n_words=1)),
        ("render", dict(list="tiles.list", n=10, begin=4, end=6, film="even")), ("render", dict(list="tiles.list", n=10, begin=6, end=8, film="odd")),
        ("error", dict(fe="even", fo="odd", list="tiles.list", list_q="tiles.list_q", n=10, taken=8, max_spp=64, **tiles)), ("compact", into),
        ("read", dict(counts="tiles.count", n_words=1))]
    regions, _ = NP.tile_layout(60)
    assert regions["list_q"][0] == 60 * 8   # (the regions are the scene's, not the range's)


def test_launch_counts():
    c = NP.constants()
    assert c == dict(block_list=2, error=1, compact=1, halves_of_no_block=2, halves=3, final_filter=3, round_raw=2, round_filtered=7)
    assert NP.call_launches(False, False, 1) == 4 and NP.call_launches(True, False, 1) == 11 and NP.call_launches(True, True, 4) == 2 + 4 * 9 + 3
    assert NP.call_launches(True, True, 2, per_render=5) == 2 + 2 * (10 + 7) + 3   # (a wavefront render is several launches)
    # a round whose block list is empty prepares and filters nothing: one launch fewer
    _, rc, launches = NP.record(True, False, W, H, N_TILES, N_TILES, 8, 64, [0, 5, 2, 0, 0])
    assert rc == 0 and launches == 2 + (2 + 2 + 2 + 2) + (2 + 3 + 2 + 2)
    _, rc, launches = NP.record(False, False, W, H, N_TILES, N_TILES, 8, 64, [5, 0], per_render=3)
    assert rc == 0 and launches == 2 * (2 * 3 + 2)


@pytest.mark.parametrize("filtered", [False, True], ids=["raw", "filtered"])
def test_a_compacted_list_longer_than_the_queue_is_refused(filtered):
    for tile_count, answer in ((48, 49), (10, 11), (10, 0xFFFFFFFF)):
        events, rc, _ = NP.record(filtered, True, W, H, N_TILES, tile_count, 8, 64, script(filtered, [answer], [6, 6]))
        assert rc == DEVICE
        assert events == expected(filtered, False, tile_count, 8, 64, [answer], [6, 6])   # round 0, and nothing after its read
    events, rc, _ = NP.record(filtered, False, W, H, N_TILES, 48, 8, 64, script(filtered, [48, 48], [6, 6, 6]))   # (as long as the queue: fine)
    assert rc == 0 and len(events) > len(expected(filtered, False, 48, 8, 64, [48], [6, 6]))


def test_a_block_list_longer_than_the_frame_has_blocks_is_refused():
    # before round 0: the two renders are on the stream already when the rule looks at the count, as ever; nothing follows them
    events, rc, _ = NP.record(True, True, W, H, N_TILES, N_TILES, 8, 64, [BLOCKS + 1, 10, 2])
    assert rc == DEVICE and events == expected(True, False, N_TILES, 8, 64, [], []) + expected(False, False, N_TILES, 8, 64, [0])[:2]
    # after round 0
    events, rc, _ = NP.record(True, True, W, H, N_TILES, N_TILES, 8, 64, [BLOCKS, 10, BLOCKS + 1, 3, 1])
    renders = [e for e in expected(True, False, N_TILES, 8, 64, [10, 3], [BLOCKS, BLOCKS + 1, 1]) if e[0] == "render"][2:4]
    assert rc == DEVICE and events == expected(True, False, N_TILES, 8, 64, [10], [BLOCKS, BLOCKS + 1]) + renders
    events, rc, _ = NP.record(True, False, W, H, N_TILES, N_TILES, 8, 64, [BLOCKS, 10, BLOCKS, 0, 0])   # (every block: fine)
    assert rc == 0


def test_an_exception_in_a_stand_in_stops_the_emulated_call_and_is_raised_again():
    """(an exception does not cross a ctypes callback by itself: tests/_noise_plan.py hands the schedule a code and raises afterwards)"""
    queue = np.array([[x, y] for y in range(2) for x in range(4)], np.uint32)
    seen = []

    def render(B, sel, begin, end, film):
        seen.append((begin, end))
        if len(seen) == 2:
            raise KeyError("no film of that range")

    def after_read(B, first, n_words):
        seen.append("read")

    with pytest.raises(KeyError):
        NP.noise_target(queue, 32, 16, 2, 8, 0.1, render, after_read)
    assert seen == [(0, 1), (1, 2)]   # nothing ran after the failure


# ---- rules

NAN, INF = float("nan"), float("inf")
# the cases of tests/test_noise_target_stub.py
RAW_INVALID = {"min1": dict(lo=1, hi=16), "min0": dict(lo=0, hi=16), "min3": dict(lo=3, hi=16), "max12": dict(lo=4, hi=12), "max_below_min": dict(lo=16, hi=8),
               "negative": dict(thr=-0.5), "nan": dict(thr=NAN), "null_even": dict(even=0), "null_odd": dict(odd=0), "same_film": dict(odd=0x1000),
               "null_samples": dict(sm=0), "null_error": dict(er=0), "null_scene": dict(scene=False)}
# those of tests/test_guide_stub.py for the filtered call add
FILTERED_INVALID = {"null_scratch": dict(scratch=0), "r0": dict(r=0), "r11": dict(r=11), "f4": dict(f=4), "k0": dict(k=0.0), "kneg": dict(k=-1.0), "knan": dict(k=NAN),
                    "kinf": dict(k=INF), "out_is_even": dict(out=0x1000), "out_is_odd": dict(out=0x2000), "out_is_scratch": dict(out=0x3000),
                    "scratch_is_even": dict(scratch=0x1000), "scratch_is_odd": dict(scratch=0x2000), "misaligned_even": dict(even=0x1004),
                    "misaligned_odd": dict(odd=0x2004), "misaligned_out": dict(out=0x6008), "misaligned_scratch": dict(scratch=0x3004)}


@pytest.mark.parametrize("filtered", [False, True], ids=["raw", "filtered"])
def test_rules_by_return_code(filtered):
    assert NP.rules(filtered) == (0, "") and NP.rules(filtered, lo=16, hi=16, thr=0.0) == (0, "")
    assert NP.rules(True, out=0x6000) == (0, "")
    for name, kw in dict(RAW_INVALID, **(FILTERED_INVALID if filtered else {})).items():
        rc, msg = NP.rules(filtered, **kw)
        assert rc == INVALID and msg, (name, rc, msg)
    for kind in (1, 2):   # Uniform, Adaptive
        assert NP.rules(filtered, sampler=kind)[0] == UNSUPPORTED
    assert NP.rules(filtered, broken=True)[0] == INVALID
    if not filtered:   # what only the filtered call looks at
        for name, kw in FILTERED_INVALID.items():
            assert NP.rules(False, **kw)[0] == 0, name


def test_the_first_refusal_wins():
    """in the calls' order: null argument, the sample counts, the threshold, the same film twice, the sampler, a broken scene; then the filtered
    call's scratch, the filter's size, radius and patch, k, and the buffers"""
    order = [(dict(sm=0), "null argument"), (dict(lo=3), "powers of two"), (dict(thr=NAN), "threshold"), (dict(odd=0x1000), "even and odd"),
             (dict(sampler=2), "LowDiscrepancy"), (dict(broken=True), "unusable"), (dict(scratch=0), "null argument"), (dict(w=0), "width and height"),
             (dict(r=11), "radius"), (dict(k=0.0), "k must"), (dict(out=0x3000), "different buffers, 16-byte aligned")]
    for i, (kw, text) in enumerate(order):
        rc, msg = NP.rules(True, **kw)
        assert text in msg and rc == (UNSUPPORTED if "sampler" in kw else INVALID), (kw, rc, msg)
        assert msg.startswith("filtered: ") or "broken" in kw   # `who` names the call, but for the scene's own sentence
        for later, _ in order[i + 1:]:
            if set(later) & set(kw):
                continue
            assert NP.rules(True, **kw, **later) == (rc, msg), (kw, later)
    assert NP.rules(False, sm=0, sampler=1)[0] == INVALID and NP.rules(False, sampler=1, broken=True)[0] == UNSUPPORTED
