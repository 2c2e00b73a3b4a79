"""The one copy of the wavefront schedule's host side (tray_rust_amd/csrc/hip/wavefront_plan.h), which libtrayhip.so and the host emulation both run:
the queue buffers' layout and its cut into views stay inside the allocations, whose sizes are the expressions wf_alloc had before the plan; a round's
launch groups come in the documented order with the documented queue aliasing; the rules (view count, max_rounds, nominal launches) by arithmetic; and
a launch of the library under the stand-in HIP runtime (tests/stubs/fakehip.c) makes, per view stream, the launches the recording Ops lists. The plan
is reached through exports of libtrayemu.so (tests/emu/wavefront_plan_record.h). No GPU."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import tray_rust_amd as T
from tray_rust_amd import scenes
import _emu as E
from _stub import kv, stub   # (stub: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOLS = [1, 63, 64, 65, 70, 128, 4096, 131072, 1 << 20]   # the last: the byte offsets need 64 bits
DEPTHS = (40, 24, 512)   # full_depth, lds_depth, n_blocks_trace of the traversal (any: the overflow columns scale with them)
QA, QB, QC, QR, NONE = 0, 1, 2, 3, 255                     # tr_wfplan::Queue; wf_record::kNone
GROUPS = ("advance", "regen", "bin", "trace", "clear_qctl", "sort", "shade_kind", "begin", "query_kind", "query")   # wf_record::Group


@pytest.fixture(scope="module")
def plan():
    h = E.emu()
    u32, ptr = C.c_uint32, C.c_void_p
    for name, restype, argtypes in [("constants", None, [ptr]), ("layout", None, [u32] * 4 + [ptr]), ("view", None, [u32] * 7 + [ptr]),
                                    ("view_count", u32, [u32] * 2), ("max_rounds", C.c_uint64, [u32] * 5), ("nominal_launches", u32, [u32]),
                                    ("round", u32, [C.c_int] * 3 + [u32, C.c_int, u32, ptr, u32])]:
        f = getattr(h, "emu_wf_plan_" + name)
        f.restype, f.argtypes = restype, argtypes
    return h


@pytest.fixture(scope="module")
def consts(plan):
    out = np.zeros(9, np.uint32)
    plan.emu_wf_plan_constants(out.ctypes.data)
    return dict(zip(("WF_SEGS", "TR_BLOCK", "WF_RAY_WORDS", "WF_QCTL_WORDS", "WF_BINS", "WF_MAT_KINDS", "WF_PIPES_MAX", "WF_POLL", "WF_FOLD_C"), (int(v) for v in out)))


def layout(plan, pool):
    out = np.zeros(13, np.uint64)
    plan.emu_wf_plan_layout(pool, *DEPTHS, out.ctypes.data)
    keys = ("q_total", "qa", "qb", "qc", "qr", "qctl_word", "bin_ctl_words", "kind_entries", "ovf_entries", "queue_bytes", "bin_ctl_bytes", "kind_bytes", "ovf_bytes")
    return dict(zip(keys, (int(v) for v in out)))


def view(plan, pool, k, n_views, n_chunks):
    out = np.zeros(7, np.uint64)
    plan.emu_wf_plan_view(pool, *DEPTHS, k, n_views, n_chunks, out.ctypes.data)
    return dict(zip(("first_chunk", "n_chunks", "seg_cap", "q_off", "qctl_word", "bin_ctl_word", "ovf_entry"), (int(v) for v in out)))


def seg_cap(c, n_chunks):   # wavefront.h: wf_seg_cap
    return (n_chunks + c["WF_SEGS"] - 1) // c["WF_SEGS"] * c["TR_BLOCK"]


def disjoint_within(ranges, end):
    """(first, size) ranges, given in rising order: none overlaps the next, and the last ends at or before `end`"""
    ends = [a + n for a, n in ranges]
    return all(e <= a for e, (a, _) in zip(ends, ranges[1:])) and ends[-1] <= end


@pytest.mark.parametrize("pool", POOLS)
def test_layout(plan, consts, pool, monkeypatch):
    monkeypatch.delenv("TRAYHIP_WF_PIPES", raising=False)
    c = consts
    segs, block, ray, qctl, pipes = c["WF_SEGS"], c["TR_BLOCK"], c["WF_RAY_WORDS"], c["WF_QCTL_WORDS"], c["WF_PIPES_MAX"]
    l = layout(plan, pool)
    # the sizes wf_alloc asked for before the plan (device_api.hip of the parent commit), written out
    q_cap, q_slack = segs * seg_cap(c, pool), pipes * segs * block
    full_depth, lds_depth, n_blocks_trace = DEPTHS
    assert l["queue_bytes"] == ((3 * ray + 1) * (q_cap + q_slack) + pipes * qctl) * 4
    assert l["bin_ctl_bytes"] == pipes * 2 * 2 * segs * c["WF_BINS"] * 4
    assert l["kind_bytes"] == c["WF_MAT_KINDS"] * (q_cap + q_slack) * 4
    assert l["ovf_bytes"] == pipes * ((full_depth - lds_depth + 1) * n_blocks_trace * block) * 4
    assert l["q_total"] == q_cap + q_slack and l["ovf_entries"] * pipes * 4 == l["ovf_bytes"] and l["bin_ctl_words"] * pipes * 4 == l["bin_ctl_bytes"]
    # the four queue kinds, then the control words of every view: disjoint, and they end at the allocation's size
    kinds = [(l["qa"], ray * l["q_total"]), (l["qb"], ray * l["q_total"]), (l["qc"], ray * l["q_total"]), (l["qr"], l["q_total"]), (l["qctl_word"], pipes * qctl)]
    assert l["qa"] == 0 and disjoint_within(kinds, l["queue_bytes"] // 4) and sum(kinds[-1]) * 4 == l["queue_bytes"]
    for used in sorted({1, max(1, pool // 2), pool}):
        for want in range(1, pipes + 1):
            n_views = plan.emu_wf_plan_view_count(used, want)
            assert 1 <= n_views <= want
            views = [view(plan, pool, k, n_views, used) for k in range(n_views)]
            # consecutive chunk ranges that partition the chunks in use; a view's segments are sized for its own chunks
            assert views[0]["first_chunk"] == 0 and sum(v["n_chunks"] for v in views) == used
            assert all(a["first_chunk"] + a["n_chunks"] == b["first_chunk"] for a, b in zip(views, views[1:]))
            assert all(v["n_chunks"] >= 1 and v["seg_cap"] == seg_cap(c, v["n_chunks"]) for v in views)
            # within each queue kind the views' entries are disjoint and end at or before q_total
            assert disjoint_within([(v["q_off"], segs * v["seg_cap"]) for v in views], l["q_total"]), (pool, used, n_views)
            # control words, bin-control words and overflow columns per view
            assert disjoint_within([(v["qctl_word"], qctl) for v in views], l["queue_bytes"] // 4) and views[0]["qctl_word"] == l["qctl_word"]
            assert disjoint_within([(v["bin_ctl_word"], l["bin_ctl_words"]) for v in views], l["bin_ctl_bytes"] // 4)
            assert disjoint_within([(v["ovf_entry"], l["ovf_entries"]) for v in views], l["ovf_bytes"] // 4)


def record(plan, fused, sorted_, bin_stages, kinds_present, anim=0):
    """one round's launch groups as (group name, stage or kind, queue read, queue filled, fused flag)"""
    out = np.zeros(5 * 64, np.uint32)
    n = plan.emu_wf_plan_round(anim, int(sorted_), int(fused), bin_stages, 1, kinds_present, out.ctypes.data, 64)
    assert n <= 64
    return [(GROUPS[g], int(s), int(a), int(b), int(f)) for g, s, a, b, f in out[:5 * n].reshape(n, 5)]


def expected_round(c, fused, sorted_, bin_stages, kinds_present):
    """the round written out: DESIGN.md section 4, "the wavefront schedule" """
    fold = c["WF_FOLD_C"] != 0
    kinds = [k for k in range(c["WF_MAT_KINDS"]) if kinds_present >> k & 1]   # TRAY_MAT_* order
    qc = NONE if fold else QC   # (the query kernels get a queue C only in builds without WF_FOLD_C)
    seq = [("advance", NONE, NONE, QA, 0), ("regen", NONE, QR, QA, 0)]
    if fold and bin_stages & 1:   # the binned copy of A lies in C, the deferred rays' records in B
        seq += [("bin", 0, QA, QC, 0), ("trace", 0, QC, QB, 0)]
    else:
        seq += [("trace", 0, QA, QB, 0)]
    seq += [("clear_qctl", NONE, NONE, NONE, 0)]   # between trace A and the first shading kernel
    if fused and sorted_ and fold:
        seq += [("sort", NONE, NONE, NONE, 0)] + [("shade_kind", k, NONE, QB, 0) for k in kinds] + [("trace", 1, QB, QC, 1)]   # (stage B is not binned here)
        return seq
    seq += [("begin", NONE, NONE, QB, 0)]
    if fold and bin_stages & 2:   # the binned copy of B lies in A, consumed by then
        seq += [("bin", 1, QB, QA, 0), ("trace", 1, QA, QC, 0)]
    else:
        seq += [("trace", 1, QB, QC, 0)]
    seq += [("query_kind", k, NONE, qc, 0) for k in kinds] if sorted_ else [("query", NONE, NONE, qc, 0)]
    if not fold:
        seq += [("trace", 2, QC, QB, 0)]
    return seq


@pytest.mark.parametrize("fused,sorted_,bin_stages,kinds_present", itertools.product((1, 0), (1, 0), (0, 1, 2, 3), (1 << 3, 0b1000101)))
def test_round_order(plan, consts, fused, sorted_, bin_stages, kinds_present):
    got = record(plan, fused, sorted_, bin_stages, kinds_present)
    assert got == expected_round(consts, fused, sorted_, bin_stages, kinds_present)
    assert got == record(plan, fused, sorted_, bin_stages, kinds_present, anim=1)   # (ANIM picks instantiations, not launches)
    # Kernel launches: bin and trace are two kernels each (histogram + scatter, traversal + fallback), the control words' clear is a memset. Against the
    # nominal count that tray_last_timing reports -- (WF_FOLD_C ? 8 : 10) + 2 per stage asked to be binned, "a kind-pure launch per material kind present
    # comes on top" --: the nominal count holds ONE launch for the shading stage (k_wf_query), which the sorted forms replace by their per-kind launches
    # (the fused form's k_wf_sort stands where k_wf_begin stood), and it counts a binned stage B that the fused form never runs.
    launches = sum(2 if g[0] in ("bin", "trace") else 0 if g[0] == "clear_qctl" else 1 for g in got)
    kind_launches = sum(g[0] in ("shade_kind", "query_kind") for g in got)
    assert kind_launches == (bin(kinds_present).count("1") if sorted_ else 0)
    is_fused = fused and sorted_ and consts["WF_FOLD_C"]
    assert launches - kind_launches == plan.emu_wf_plan_nominal_launches(bin_stages) - (1 if sorted_ else 0) - (2 if is_fused and bin_stages & 2 else 0)


def test_rules(plan, consts, monkeypatch):
    monkeypatch.delenv("TRAYHIP_WF_PIPES", raising=False)
    c = consts
    views = plan.emu_wf_plan_view_count
    edge = (24 << 20) // c["TR_BLOCK"]   # 24 M slots
    assert (views(edge - 1, 0), views(edge, 0), views(edge + 1, 0)) == (2, 1, 1)
    assert [views(edge, r) for r in (1, 2, 3, 4, 5, 100)] == [1, 2, 3, 4, 4, 4]   # tray_scene_set_wavefront, at most WF_PIPES_MAX
    assert c["WF_PIPES_MAX"] == 4
    # the clamp: a view has at least WF_SEGS chunks, and there is always one view
    segs = c["WF_SEGS"]
    assert [views(n, 0) for n in (1, segs - 1, segs, 2 * segs - 1, 2 * segs)] == [1, 1, 1, 1, 2]
    assert [views(3 * segs, r) for r in (1, 2, 3, 4)] == [1, 2, 3, 3]
    monkeypatch.setenv("TRAYHIP_WF_PIPES", "3")
    assert (views(edge, 0), views(edge, 1), views(2 * segs, 0), views(1, 0)) == (3, 3, 2, 1)
    monkeypatch.delenv("TRAYHIP_WF_PIPES")

    def parent_max_rounds(tile_count, n_chunks, n, slice_shift, max_depth):   # launch_wavefront of the parent commit; tile_count: work items
        tiles_per_chunk = (tile_count + n_chunks - 1) // n_chunks
        return tiles_per_chunk * (((n + (1 << slice_shift) - 1 >> slice_shift) + 3) // 4 * ((2 if c["WF_FOLD_C"] else 1) * max_depth + 3) + 4) + 2 * c["WF_POLL"]

    for args in [(64, 4, 16, 0, 5), (64, 64, 16, 0, 5), (256, 4, 64, 2, 5), (129600, 129600, 1024, 4, 15), (130, 7, 33, 1, 3), (1 << 22, 1 << 19, 512, 4, 8)]:
        assert plan.emu_wf_plan_max_rounds(*args) == parent_max_rounds(*args), args
    assert c["WF_POLL"] == 16 and [plan.emu_wf_plan_nominal_launches(b) for b in range(4)] == [n + (8 if c["WF_FOLD_C"] else 10) for n in (0, 2, 2, 4)]


DRIVER = r'''
import sys
sys.path.insert(0, %(root)r)
import tray_rust_amd as T
scene, rt, spp, fi = T.Scene.load_file(%(path)r)
hip = T.Hip(0, seed=4)
hip.render(scene, rt, T.Config(".", "s", spp, 1, fi, (0, 0)))
print("DONE views=%%d" %% hip.schedule(scene)["views"])
'''
KERNELS = {"advance": ["k_wf_advance"], "regen": ["k_wf_regen"], "bin": ["k_wf_bin_hist", "k_wf_bin_scatter"], "trace": ["k_wf_trace_dyn", "k_wf_trace_fallback"],
           "clear_qctl": [], "sort": ["k_wf_sort"], "shade_kind": ["k_wf_shade_kind"], "begin": ["k_wf_begin"], "query_kind": ["k_wf_query_kind"], "query": ["k_wf_query"]}


@pytest.mark.parametrize("fused", ["1", "0"])
def test_the_library_runs_the_plan(plan, consts, stub, tmp_path, fused, built):
    """a static scene, two views: each view's stream carries WF_POLL rounds (the stand-in's poll then reads "all done") of the recorded round"""
    scenes.write_assets(str(tmp_path), cornell=(128, 128, 16))   # 256 tiles, one work item each: 256 chunks in use, enough for two views
    path = os.path.join(str(tmp_path), "cornell_box.json")
    sp = E.scene_plan(T.Scene.load_file(path)[0].flatten(0))
    env = {k: None for k in ("TRAYHIP_WF_BIN", "TRAYHIP_WF_SLICES", "TRAYHIP_XF_TABLE", "FAKEHIP_TILE_KERNEL", "FAKEHIP_MALLOC_MAX")}
    out, log = stub(DRIVER % {"root": ROOT, "path": path}, tmp_path, FAKEHIP_DEVICES=1, FAKEHIP_WF_DONE=1, FAKEHIP_FREE_BYTES=4 << 30, TRAYHIP_MODE="wave",
                    TRAYHIP_WF_SLOTS=65536, TRAYHIP_WF_PIPES=2, TRAYHIP_WF_FUSED=fused, **env)
    assert "DONE views=2" in out.stdout, out.stdout + out.stderr
    streams = {}
    for l in log:
        m = re.search(r"k_wf_[a-z_]+", l) if l.startswith("launch") else None
        if m:
            streams.setdefault(kv(l)["stream"], []).append(m.group(0))
    sorted_ = not sp["feat"] & 8   # dev_bsdf.h: FEAT_TEX
    round_ = [k for g in record(plan, int(fused), sorted_, 0, sp["mat_kinds_present"]) for k in KERNELS[g[0]]]
    assert sorted_ and ("k_wf_shade_kind" in round_) == (fused == "1") and ("k_wf_begin" in round_) == (fused == "0")
    assert len(streams) == 2 and all(seq == round_ * consts["WF_POLL"] for seq in streams.values()), streams
