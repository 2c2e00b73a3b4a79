"""The one copy of the decisions about a device scene's launch buffers -- wavefront pool, per-path transform cache, transform table
(tray_rust_amd/csrc/hip/launch_buffers_plan.h) --, run here without the library and without a GPU: its sizes and rules against the expressions
device_api.hip had before the plan, written out below; the five scripted sequences of tests/test_launch_buffers_stub.py through a scripted Ops
(tests/emu/launch_buffers_plan_record.h), which must give the numbers the whole library gives under the stand-in runtime; a sweep of prepare over
memory, requests and prior states that checks the invariants the header states; ADVICE round 6's sequence by name. The plan is reached through
exports of libtrayemu.so."""
import ctypes as C
import itertools

import numpy as np
import pytest

import tray_rust_amd as T
from tray_rust_amd import scenes
import _emu as E
from _launch_buffer_sequences import ENV, EXPECTED, FREE_BYTES, STEPS, TR_XF_REC, film_size

GiB = 1 << 30
CONSTANTS = ("TR_BLOCK", "TR_XF_REC", "TR_XF_WORDS", "F_COUNT", "WF_RAY_WORDS", "WF_MAT_KINDS", "ROWBIN_SIZE", "sizeof_WfChunk", "WF_MAX_SLICES", "WF_TRACE_WAVES",
             "WF_SLOTS", "XF_TABLE_MIN_SAMPLES", "time_indices", "TRAY_E_NOMEM", "TRAY_E_DEVICE")
PLAN_ENV = ("TRAYHIP_WF_SLOTS", "TRAYHIP_XF_CACHE_BYTES", "TRAYHIP_XF_TABLE", "TRAYHIP_WF_LDS_DEPTH")
CALLS = ("free_bytes", "grant_cache", "grant_table", "grant_pool", "drop", "synchronise", "table_build", "table_wait", "refusal", "no_pool", "cache_short")   # lb_record::Call
POOL, CACHE, TABLE_PART = 1, 2, 4   # tr_lbplan::kPool, kCache, kTable


@pytest.fixture(scope="module")
def plan():
    h = E.emu()
    u32, u64, i, ptr = C.c_uint32, C.c_uint64, C.c_int, C.c_void_p
    for name, restype, argtypes in [("constants", None, [ptr]), ("sizes", None, [u32, u32, u32, i, u32, u32, ptr]), ("slot_wish", u32, [u32, u32]),
                                    ("slot_fit", u32, [u32, u64, u64, u32]), ("cache_budget", u32, [u32, u32, u64]), ("table_wanted", i, [i, u64, i, i]),
                                    ("trace_depths", None, [u32, ptr]), ("wish_changed", i, [i, u32, u32, u32]), ("new", ptr, []), ("delete", None, [ptr]),
                                    ("facts", None, [ptr, ptr]), ("table_request", None, [ptr, i]), ("memory", None, [ptr, u64, i, u64]), ("frame", i, [ptr]),
                                    ("prepare", i, [ptr, u64]), ("set_wavefront", None, [ptr, u32]), ("state", None, [ptr, ptr]),
                                    ("broken", u32, [ptr, i, ptr, u32]), ("log", u32, [ptr, ptr, u32]), ("sweep", u64, [ptr, ptr, u32])]:
        f = getattr(h, "emu_lb_plan_" + name)
        f.restype, f.argtypes = restype, argtypes
    return h


@pytest.fixture(scope="module")
def c(plan):
    out = np.zeros(len(CONSTANTS), np.uint64)
    plan.emu_lb_plan_constants(out.ctypes.data)
    return dict(zip(CONSTANTS, (int(v) for v in out.astype(np.int64))))


@pytest.fixture
def env(monkeypatch):
    """sets the plan's environment overrides for a test (None: unset), none of them inherited"""
    def set_(**kw):
        for k in PLAN_ENV:
            monkeypatch.delenv(k, raising=False)
        for k, v in kw.items():
            if v is not None:
                monkeypatch.setenv(k, str(v))
    set_()
    return set_


# ---- the rules as device_api.hip had them (wf_bytes_per_slot, wf_slot_wish, wf_slot_fit, xf_cache_budget, launch_prepare's `want`, wf_alloc's lds_depth)

def bytes_per_slot(c):
    return c["F_COUNT"] * 4 + (3 * c["WF_RAY_WORDS"] + 1) * 4 + c["WF_MAT_KINDS"] * 4 + (c["ROWBIN_SIZE"] * 4 + c["sizeof_WfChunk"]) // c["TR_BLOCK"]


def slot_wish(c, tiles, req, env_slots):
    b = c["TR_BLOCK"]
    n = c["WF_SLOTS"]
    if req:
        n = max(req, 64 * b) // b * b
    if env_slots is not None:
        n = max(256, env_slots) // b * b
    return min(n, max(tiles, 1) * b * c["WF_MAX_SLICES"])


def slot_fit(c, tiles, slots, free, req, env_slots):
    b = c["TR_BLOCK"]
    slots = min(slots, max(free // 3 // bytes_per_slot(c) // b * b, 64 * b))
    per_tile_level = max(tiles, 1) * b
    if slots > per_tile_level and not req and env_slots is None:
        fit = per_tile_level
        while fit * 2 <= slots and fit * 2 <= per_tile_level * c["WF_MAX_SLICES"]:
            fit *= 2
        slots = fit
    return slots


def cache_budget(c, tiles, movers, free, env_slots, env_cache):
    b = c["TR_BLOCK"]
    budget = free // 5 * 2 if env_cache is None else max(0, env_cache)
    fit = budget // (movers * c["TR_XF_REC"] * 4) // b * b
    return slot_fit(c, tiles, min(slot_wish(c, tiles, 0, env_slots), max(fit, 64 * b)), free, 0, env_slots)


TILES, REQUESTS, FREE, MOVERS = (1, 64, 256, 32400), (0, 1, 32768, 1 << 27), (0, GiB, 4 * GiB, 256 * GiB), (1, 4, 11)
CACHE_ENV = 4 * TR_XF_REC * 4 * 32768


@pytest.mark.parametrize("env_slots", [None, 65536, 100])
def test_slot_wish_and_fit(plan, c, env, env_slots):
    env(TRAYHIP_WF_SLOTS=env_slots)
    for tiles, req in itertools.product(TILES, REQUESTS):
        wish = slot_wish(c, tiles, req, env_slots)
        assert plan.emu_lb_plan_slot_wish(tiles, req) == wish, (tiles, req)
        assert wish % c["TR_BLOCK"] == 0 and wish >= c["TR_BLOCK"]
        for free in FREE:
            assert plan.emu_lb_plan_slot_fit(tiles, wish, free, req) == slot_fit(c, tiles, wish, free, req, env_slots), (tiles, req, free)


@pytest.mark.parametrize("env_slots", [None, 65536])
@pytest.mark.parametrize("env_cache", [None, CACHE_ENV, 0])
def test_cache_budget(plan, c, env, env_slots, env_cache):
    env(TRAYHIP_WF_SLOTS=env_slots, TRAYHIP_XF_CACHE_BYTES=env_cache)
    for tiles, free, movers in itertools.product(TILES, FREE, MOVERS):
        lanes = cache_budget(c, tiles, movers, free, env_slots, env_cache)
        assert plan.emu_lb_plan_cache_budget(tiles, movers, free) == lanes, (tiles, free, movers)
        assert lanes % c["TR_BLOCK"] == 0 and lanes >= min(64, max(tiles, 1)) * c["TR_BLOCK"]   # (64 chunks, or the film's one chunk per tile)


def test_the_pool_goes_when_the_wish_changes(plan, c, env):
    for tiles, before, after in itertools.product(TILES, REQUESTS, REQUESTS):
        changed = slot_wish(c, tiles, before, None) != slot_wish(c, tiles, after, None)
        assert plan.emu_lb_plan_wish_changed(1, tiles, before, after) == int(changed), (tiles, before, after)
        assert plan.emu_lb_plan_wish_changed(0, tiles, before, after) == 0   # (no pool: nothing to drop)
    env(TRAYHIP_WF_SLOTS=65536)   # (the environment's word is the wish whatever is requested)
    assert not any(plan.emu_lb_plan_wish_changed(1, 256, before, after) for before, after in itertools.product(REQUESTS, REQUESTS))


@pytest.mark.parametrize("env_table", [None, 0, 1])
def test_table_rule(plan, c, env, env_table):
    env(TRAYHIP_XF_TABLE=env_table)
    at = c["XF_TABLE_MIN_SAMPLES"]
    assert at == 30000000
    for req, samples, built, exists in itertools.product((-1, 0, 1), (at - 1, at), (0, 1), (0, 1)):
        want = req if env_table is None else env_table
        if want < 0:
            want = int(samples >= at or built or exists)
        assert plan.emu_lb_plan_table_wanted(req, samples, built, exists) == want, (req, samples, built, exists)


@pytest.mark.parametrize("env_depth", [None, 1, 5, 1000])
def test_trace_lds_depth(plan, c, env, env_depth):
    env(TRAYHIP_WF_LDS_DEPTH=env_depth)
    for words in (0, 7, 8, 9, 24, 40, 41, 200):
        full = max(words, 8)
        lds = min(full, (160 * 1024 // c["WF_TRACE_WAVES"]) // (c["TR_BLOCK"] * 4))
        if env_depth is not None:
            lds = min(full, max(1, env_depth))
        out = np.zeros(2, np.uint32)
        plan.emu_lb_plan_trace_depths(words, out.ctypes.data)
        assert tuple(out) == (full, lds), words


def test_byte_figures(plan, c):
    assert c["time_indices"] == 1 << 24 and c["TR_XF_REC"] == TR_XF_REC
    for slots, movers, wavefront, lanes, cap in [(0, 0, 1, 0, 0), (256, 1, 1, 256, 1), (32768, 4, 1, 32768, 5), (1 << 20, 4, 0, 1 << 18, 5), (1 << 27, 11, 1, 1 << 27, 12),
                                                 (0xffffff00, 64, 1, 0xffffff00, 64)]:   # (the last two: every figure needs 64 bits)
        chunks = slots // c["TR_BLOCK"]
        out = np.zeros(6, np.uint64)
        plan.emu_lb_plan_sizes(slots, chunks, movers, wavefront, lanes, cap, out.ctypes.data)
        assert [int(v) for v in out] == [c["F_COUNT"] * slots * 4, bytes_per_slot(c), chunks * c["sizeof_WfChunk"], chunks * c["ROWBIN_SIZE"] * 4,
                                        movers * (c["TR_XF_REC"] if wavefront else c["TR_XF_WORDS"]) * lanes * 4, (1 << 24) * cap * c["TR_XF_REC"] * 4]


# ---- the procedures through the scripted Ops

class Session:
    """a device scene's launch buffers as the plan alone sees them (lb_record::Session)"""
    STATE = ("pool_slots", "xf_cache_bytes", "xf_table_bytes", "transform_table", "cache_lanes", "table_stride", "table_cap", "table_built", "wf_shrunk")

    def __init__(self, plan, free=FREE_BYTES, max_grant=None):
        self.plan, self.h = plan, plan.emu_lb_plan_new()
        self.req_slots, self.table_req, self.rc = 0, -1, 0
        self.memory(free, max_grant)

    def close(self):
        self.plan.emu_lb_plan_delete(self.h)

    def memory(self, free, max_grant):
        """free: bytes, or None if the device cannot be asked; max_grant: the largest allocation granted, None: any"""
        self.plan.emu_lb_plan_memory(self.h, free or 0, free is not None, (1 << 64) - 1 if max_grant is None else max_grant)

    def frame(self, n_tiles, n_moving, animated=True, camera_animated=True, xf_movable=0, stack_bytes=8192, wavefront=True, tile_workgroups=1024):
        v = np.array([n_tiles, tile_workgroups, wavefront, animated, n_moving, stack_bytes, 24, xf_movable, camera_animated, self.req_slots, self.table_req], np.int64)
        self.plan.emu_lb_plan_facts(self.h, v.ctypes.data)
        self.rc = self.plan.emu_lb_plan_frame(self.h)
        return self.rc

    def set_transform_table(self, mode):
        self.table_req = mode
        self.plan.emu_lb_plan_table_request(self.h, mode)

    def set_wavefront(self, req_slots):
        self.req_slots = req_slots
        self.plan.emu_lb_plan_set_wavefront(self.h, req_slots)

    def prepare(self, samples):
        self.rc = self.plan.emu_lb_plan_prepare(self.h, samples)
        return self.rc

    def state(self):
        out = np.zeros(len(self.STATE), np.uint64)
        self.plan.emu_lb_plan_state(self.h, out.ctypes.data)
        return dict(zip(self.STATE, (int(v) for v in out)))

    def broken(self, launched):
        """'' or the invariant of launch_buffers_plan.h that does not hold (launched: the last prepare returned TRAY_OK)"""
        msg = C.create_string_buffer(256)
        self.plan.emu_lb_plan_broken(self.h, int(launched), msg, 256)
        return msg.value.decode()

    def log(self):
        n = self.plan.emu_lb_plan_log(self.h, None, 0)
        out = np.zeros((n, 3), np.uint64)
        self.plan.emu_lb_plan_log(self.h, out.ctypes.data, n)
        return [(CALLS[int(call)], int(a), int(b)) for call, a, b in out]


@pytest.fixture
def session(plan):
    made = []

    def new(**kw):
        made.append(Session(plan, **kw))
        return made[-1]
    yield new
    for s in made:
        s.close()


def run_steps(session, tmp_path, seq, monkeypatch):
    """STEPS[seq] over the plan alone: the names the statements use are bound to a Session with the facts of the sequence's moving_box, the memory
    settings of the stand-in runtime and the sequence's environment; returns what tests/test_launch_buffers_stub.py's run() returns, by number"""
    size = film_size(seq)
    scene, _, _, _ = T.Scene.load_file(scenes.write_moving_box(str(tmp_path), width=size, height=size, samples=16))
    n_tiles = (size // 8) ** 2
    for k in PLAN_ENV:
        monkeypatch.delenv(k, raising=False)
    settings = dict(ENV[seq])
    for k, v in settings.items():
        if k.startswith("TRAYHIP_"):
            monkeypatch.setenv(k, v)
    limit = settings.get("FAKEHIP_MALLOC_MAX")
    s = session(free=FREE_BYTES, max_grant=None if limit is None else int(limit))
    shown = []

    class Hip:   # tray_rust_amd.Hip's three calls of the sequences
        def set_transform_table(self, _scene, mode):
            s.set_transform_table(mode)

        def set_wavefront(self, _scene, pool_slots):
            s.set_wavefront(pool_slots)

    class Environ(dict):   # os.environ: the stand-in runtime's malloc limit
        def __setitem__(self, k, v):
            assert k == "FAKEHIP_MALLOC_MAX"
            s.memory(FREE_BYTES, int(v))

    class Os:
        environ = Environ()

    def show(label):
        st = s.state()
        assert s.broken(launched=label.startswith("launch")) == "", (seq, label, st)
        shown.append((label, tuple(st[k] for k in ("pool_slots", "xf_cache_bytes", "xf_table_bytes", "transform_table"))))

    def frame(f):
        flat = scene.flatten(f)
        p = E.scene_plan(flat)
        assert s.frame(n_tiles, p["n_moving"], bool(p["animated"]), bool(flat.contents.camera.animated), p["xf_movable"], p["stack_bytes"]) == 0
        show("frame%d" % f)

    def launch(f):
        assert s.prepare(n_tiles * 64 * 16) == 0, s.log()[-4:]
        show("launch%d" % f)

    names = {"frame": frame, "launch": launch, "show": show, "hip": Hip(), "scene": None, "os": Os}
    for step in STEPS[seq]:
        exec(step, names)
    return shown, s


@pytest.mark.parametrize("seq", sorted(STEPS))
def test_the_sequences_give_the_numbers_the_library_gives(plan, session, tmp_path, monkeypatch, seq):
    shown, _ = run_steps(session, tmp_path, seq, monkeypatch)
    assert shown == EXPECTED[seq]


def test_advice_round_6_a_pool_larger_than_the_cache_gets_a_cache_for_every_slot(plan, c, session, tmp_path, monkeypatch):
    """ADVICE.md round 6, second finding: a per-path launch leaves a cache of 32 768 lanes, tray_scene_set_wavefront frees the pool, a table launch allocates
    a pool of 131 072 slots, the table goes off: the next launch, which indexes the cache by pool slot, must have a record for every one of them"""
    shown, s = run_steps(session, tmp_path, "a", monkeypatch)
    per_lane = 4 * TR_XF_REC * 4
    (_, first), (_, dropped), (_, table), (_, last) = shown[1:]
    assert first[:2] == (32768, 32768 * per_lane) and dropped[:2] == (0, 32768 * per_lane)
    assert table[0] == 131072 and table[3] == 1 and table[1] == 32768 * per_lane       # (the table launch reads no cache: it may stay small)
    assert last[0] == 131072 and last[3] == 0 and last[1] >= 131072 * per_lane and s.state()["cache_lanes"] >= 131072
    calls = s.log()
    drop = max(i for i, call in enumerate(calls) if call[0] == "drop")
    assert calls[drop][1] == CACHE and calls[drop - 1][0] == "synchronise"                # (the small cache goes behind a synchronise ...)
    assert calls[drop + 1][:2] == ("grant_cache", 131072)                                # (... and comes back with the pool's slots)


def test_cache_ensure_synchronises_before_each_drop_and_table_ensure_does_not(plan, session):
    s = session(free=256 * GiB)
    s.set_transform_table(1)
    assert s.frame(64, 4, xf_movable=5) == 0 and s.prepare(65536) == 0       # a table with room for five records
    assert s.frame(64, 7, xf_movable=5) == 0                                  # the next frame moves seven instances + the camera
    before = len(s.log())
    assert s.prepare(65536) == 0 and s.state()["table_cap"] == 8
    calls = s.log()[before:]
    assert ("drop", TABLE_PART, 0) in calls and not any(call[0] == "synchronise" for call in calls)
    # a pool sized for table launches, larger than the cache: a cache for all of it does not fit in two fifths of the free memory, so the pool goes behind
    # a synchronise and comes back with the cache's lanes (the other drop of cache_ensure, the too-small cache's, is ADVICE round 6's case above)
    s = session(free=GiB)
    s.set_transform_table(0)
    assert s.frame(32400, 4, xf_movable=5) == 0 and s.prepare(65536) == 0
    lanes = s.state()["cache_lanes"]
    assert s.state()["pool_slots"] == lanes
    s.set_wavefront(1 << 26)
    s.set_transform_table(1)
    s.memory(256 * GiB, None)
    assert s.prepare(65536) == 0 and s.state()["pool_slots"] == 1 << 26
    s.set_transform_table(0)
    s.memory(GiB, None)
    before = len(s.log())
    assert s.prepare(65536) == 0
    calls = s.log()[before:]
    assert [call[:2] for call in calls] == [("free_bytes", 1), ("synchronise", 0), ("drop", POOL), ("refusal", 0), ("grant_pool", lanes)]
    assert s.state()["pool_slots"] == lanes and s.broken(launched=True) == ""


def test_what_a_device_that_cannot_be_asked_counts_as(plan, c, session):
    """16 GiB free where the pool and the cache's budget are sized, nothing free where cache_ensure weighs a cache for the pool, room where table_ensure
    applies the third-of-free rule"""
    s = session(free=None)
    s.set_wavefront(1 << 27)   # (a request bounds the pool, not the cache's budget, and is not cut to the film's tiles x 2^k)
    assert s.frame(32400, 4, xf_movable=5) == 0
    assert s.state()["cache_lanes"] == cache_budget(c, 32400, 4, 16 * GiB, None, None)
    assert s.prepare(c["XF_TABLE_MIN_SAMPLES"]) == 0 and s.state()["transform_table"] == 1      # (nobody asked for the table: the own rule, and there is room)
    assert s.state()["pool_slots"] == slot_fit(c, 32400, slot_wish(c, 32400, 1 << 27, None), 16 * GiB, 1 << 27, None)
    s.set_transform_table(0)
    assert s.state()["pool_slots"] > s.state()["cache_lanes"]
    before = len(s.log())
    assert s.prepare(65536) == 0
    assert [call[0] for call in s.log()[before:]][:3] == ["free_bytes", "synchronise", "drop"]  # (the pool goes: a cache for it fits in "nothing")
    assert s.broken(launched=True) == ""


def test_the_table_takes_at_most_a_third_of_free_memory_only_when_nobody_asked_for_it(plan, c, session):
    table = (1 << 24) * 5 * TR_XF_REC * 4
    for req, want_table in ((-1, 0), (1, 1)):
        s = session(free=3 * table - 3)
        s.set_transform_table(req)
        assert s.frame(64, 4, xf_movable=5) == 0 and s.prepare(c["XF_TABLE_MIN_SAMPLES"]) == 0
        assert s.state()["transform_table"] == want_table and s.broken(launched=True) == ""
    s = session(free=3 * table)
    assert s.frame(64, 4, xf_movable=5) == 0 and s.prepare(c["XF_TABLE_MIN_SAMPLES"]) == 0 and s.state()["transform_table"] == 1


def test_no_pool_is_nomem_with_the_handle_as_it_was(plan, c, session):
    s = session(free=256 * GiB, max_grant=1 << 20)
    assert s.frame(64, 0, animated=False, camera_animated=False) == 0
    assert s.prepare(65536) == c["TRAY_E_NOMEM"]      # (halved from the film's 262 144 slots down to 64 chunks: 4 MiB of pool fields)
    calls = s.log()
    assert calls[-1] == ("no_pool", 64 * c["TR_BLOCK"], 0) and s.state()["pool_slots"] == 0 and s.broken(launched=False) == ""


def test_invariant_sweep(plan):
    """lb_record::sweep (tests/emu/launch_buffers_plan_record.h): prepare, and a second prepare with the table request turned round, over free bytes x
    largest grant x table request x sample count x movers x film x prior state. After every prepare that returns TRAY_OK a launch that reads the cache has
    lanes >= pool slots and the bytes for them, the pool's slots are a multiple of TR_BLOCK and at most the wish, a table launch has a built table with
    stride <= cap; after every return every grant is owned by the state or was dropped exactly once and nothing dropped is still named"""
    failures, msg = C.c_uint64(0), C.create_string_buffer(512)
    cases = plan.emu_lb_plan_sweep(C.byref(failures), msg, 512)
    assert cases == 6 * 5 * 3 * 2 * 2 * 2 * 2 * 7
    assert failures.value == 0, msg.value.decode()
