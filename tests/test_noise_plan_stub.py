"""The later rounds of the two noise-target calls through the real library against the stand-in runtime (tests/stubs/fakehip.c), as
tests/test_guide_stub.py does round 0: with FAKEHIP_NOISE_KEEP="10,3" the stand-in tile compaction keeps the first 10 tiles of the queue after round
0, the first 3 after round 1 and none after round 2, so the library's own loop switches to the compacted list, reads both counts and makes the block
list from the flags. The logged launches are the sequence written out by hand below, they are what the recording Ops of
tests/emu/noise_plan_record.h lists for the same counts, and TrayKernelTiming counts them. With FAKEHIP_NOISE_KEEP="49,49" the compaction reports more
tiles than the queue has: both calls refuse with TRAY_E_DEVICE after round 0, launch nothing more and leave no timing behind."""
import os

import _noise_plan as NP
from _stub import events as all_events, stub   # (stub: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, N_TILES, SPP, LO = 64, 48, 48, 64, 8
F_ = 3   # (radius 7, patch 3: the recording Ops's filter)
KEEP = [10, 3]

DRIVER = r'''
import ctypes as C, os, sys
sys.path.insert(0, %(root)r)
import tray_rust_amd as T
from tray_rust_amd import _lib as L, scenes
lib = T.lib()
W, H = 64, 48
al = lambda b: (C.addressof(b) + 15) & ~15
films = [C.create_string_buffer(W * H * 16 + 32) for _ in range(3)]
even, odd, out = (al(b) for b in films)
scr = C.create_string_buffer(int(lib.tray_noise_target_filtered_scratch_bytes(W, H)) + 32)
smp, err = (C.c_uint32 * 48)(), (C.c_float * 48)()
d = %(tmp)r
scenes.write_assets(d, cornell=(W, H, 16))
scene, rt, spp, fi = T.Scene.load_file(os.path.join(d, "cornell_box.json"))
dev = scene.device_scene(0, 0)
t = L.TrayKernelTiming()
print("RC_RAW", lib.tray_render_noise_target_device(dev, 0, 0, 8, 64, 0.05, 3, even, odd, smp, err, None))
print("TIMING_RAW", lib.tray_last_timing(dev, C.byref(t)), t.launches)
print("RC_FILTERED", lib.tray_render_noise_target_filtered_device(dev, 0, 0, 8, 64, 0.05, 3, even, odd, 7, 3, 0.45, out, al(scr), smp, err, None))
print("TIMING_FILTERED", lib.tray_last_timing(dev, C.byref(t)), t.launches)
print("DONE")
'''

PX = lambda w, h: (w * h + 255) // 256
BLOCKS = lambda w, h: ((w + 31) // 32) * ((h + 15) // 16)


def by_hand(filtered):
    """the launches of a call over the 48 tiles whose compaction keeps 10, 3 and no tile, as all_events reports them (streams cut off)"""
    prepare = [("denoise", "prepare", 0, PX(W, H), 256), ("denoise", "prepare", 1, PX(W, H), 256)]
    block_list = [("guide", "k_guide_mark", -1, (N_TILES + 255) // 256, 256), ("guide", "k_guide_compact", -1, 1, 1024)]   # (over the whole queue, every round)
    ev = block_list if filtered else []
    for n, (lo, mid, hi) in zip((48, 10, 3), ((0, 4, 8), (8, 12, 16), (16, 24, 32))):
        ev = ev + [("range", lo, mid, n, SPP, n, 1), ("range", mid, hi, n, SPP, n, 1)]
        if filtered:   # (the stand-in block compaction answers "every block")
            ev = ev + prepare + [("guide", "k_dn_filter_halves", F_, BLOCKS(W, H), 512)]
        ev = ev + [("noise", "error", (n + 3) // 4, 256), ("noise", "compact", 1, 1024)] + (block_list if filtered else [])
    return ev + (prepare + [("denoise", "filter", F_, BLOCKS(W, H), 512)] if filtered else [])


def launches_of(recorded):
    """the launches the library makes for the recording Ops's groups, in all_events' form"""
    prepare = [("denoise", "prepare", 0, PX(W, H), 256), ("denoise", "prepare", 1, PX(W, H), 256)]
    ev = []
    for group, a in recorded:
        if group == "render":
            ev.append(("range", a["begin"], a["end"], a["n"], SPP, a["n"], 1))
        elif group == "block_list":
            ev += [("guide", "k_guide_mark", -1, (a["n"] + 255) // 256, 256), ("guide", "k_guide_compact", -1, 1, 1024)]
        elif group == "halves":
            ev += prepare + [("guide", "k_dn_filter_halves", a["patch"], a["n_blocks"], 512)]
        elif group == "error":
            ev.append(("noise", "error", (a["n"] + 3) // 4, 256))
        elif group == "compact":
            ev.append(("noise", "compact", 1, 1024))
        elif group == "final_filter":
            ev += prepare + [("denoise", "filter", a["patch"], BLOCKS(W, H), 512)]
    return ev


def test_a_compacted_list_longer_than_the_queue_is_refused_by_the_library(stub, tmp_path):
    out, log = stub(DRIVER % {"root": ROOT, "tmp": str(tmp_path)}, tmp_path, FAKEHIP_DEVICES=1, FAKEHIP_TILE_KERNEL=1, FAKEHIP_NOISE_KEEP="49,49")
    assert "DONE" in out.stdout and "RC_RAW -5" in out.stdout and "RC_FILTERED -5" in out.stdout, out.stdout + out.stderr   # TRAY_E_DEVICE
    # the renders before the refusal recorded a timing of their own: the failed call's is none (TRAY_E_INVALID, "no launch recorded")
    assert "TIMING_RAW -1 0" in out.stdout and "TIMING_FILTERED -1 0" in out.stdout, out.stdout
    ev = [e[:5] if e[0] in ("guide", "denoise") else e for e in all_events(log)]
    nb = BLOCKS(W, H)
    want = []
    for rule, script in ((False, [49]), (True, [nb, 49, nb])):
        recorded, rc, _ = NP.record(rule, True, W, H, N_TILES, N_TILES, LO, SPP, script)
        assert rc == -5
        want += launches_of(recorded)
    assert len(want) == 4 + 11 and ev == want, ev   # round 0 of each call and nothing after its read: no second round, no final filter


def test_the_later_rounds_of_both_calls(stub, tmp_path):
    out, log = stub(DRIVER % {"root": ROOT, "tmp": str(tmp_path)}, tmp_path, FAKEHIP_DEVICES=1, FAKEHIP_TILE_KERNEL=1, FAKEHIP_NOISE_KEEP=",".join(map(str, KEEP)))
    assert "DONE" in out.stdout and "RC_RAW 0" in out.stdout and "RC_FILTERED 0" in out.stdout, out.stdout + out.stderr
    ev = [e[:5] if e[0] in ("guide", "denoise") else e for e in all_events(log)]
    raw, filtered = by_hand(False), by_hand(True)
    assert ev == raw + filtered, ev
    # the plan's schedule, recorded for the same counts (the stand-in block compaction: all six blocks, every time)
    nb = BLOCKS(W, H)
    for rule, hand, script in ((False, raw, KEEP + [0]), (True, filtered, [nb] + [w for m in KEEP + [0] for w in (m, nb)])):
        recorded, rc, launches = NP.record(rule, True, W, H, N_TILES, N_TILES, LO, SPP, script)
        assert rc == 0 and launches_of(recorded) == hand
        assert launches == len(hand)
        assert f"TIMING_{'FILTERED' if rule else 'RAW'} 0 {len(hand)}" in out.stdout, out.stdout   # TrayKernelTiming counts every launch of the call
