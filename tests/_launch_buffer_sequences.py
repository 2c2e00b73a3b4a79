"""The scripted sequences of launches, tray_scene_set_wavefront, tray_scene_set_transform_table and frame updates over a device scene's launch buffers,
and tray_last_schedule's numbers after every step. tests/test_launch_buffers_stub.py runs them through Python, the whole library and the stand-in HIP
runtime; tests/test_launch_buffers_plan.py runs the same steps through csrc/hip/launch_buffers_plan.h alone with a scripted Ops: two routes to one set
of numbers. The scene is tray_rust_amd.scenes' moving_box at 16 spp; a step is a Python statement over frame(f), launch(f), show(label), hip, scene, os."""
TR_XF_REC = 32   # floats per record of the cache and the table (dev_anim.h)
KEYS = ("pool_slots", "xf_cache_bytes", "xf_table_bytes", "transform_table")
FREE_BYTES = 4 << 30   # what the device reports free (FAKEHIP_FREE_BYTES)


def film_size(seq):
    """width and height of the sequence's film"""
    return 128 if seq == "e" else 64


STEPS = {
    # the round-6 review's sequence (second finding): a per-path launch leaves a cache of L lanes, tray_scene_set_wavefront frees the pool,
    # a table launch allocates a pool larger than L, the table goes off -- the next launch must not index the cache past its L lanes
    "a": ["frame(0)", "hip.set_transform_table(scene, 0)", "launch(0)", "hip.set_wavefront(scene, 131072)", "show('set_wavefront')",
          "hip.set_transform_table(scene, 1)", "launch(0)", "hip.set_transform_table(scene, 0)", "launch(0)"],
    # a sequence that renders through the table: the pool and the table's buffer are there before every new frame's first launch
    "b": ["frame(0)", "hip.set_transform_table(scene, 1)", "launch(0)", "frame(1)", "launch(1)", "frame(2)", "launch(2)"],
    # ... and one that evaluates per path: the cache and the pool are handed on
    "c": ["frame(0)", "hip.set_transform_table(scene, 0)", "launch(0)", "frame(1)", "launch(1)", "frame(2)", "launch(2)"],
    # another pool size: the buffers go at once and come back at the new size with the next launch
    "d": ["frame(0)", "hip.set_transform_table(scene, 1)", "launch(0)", "hip.set_wavefront(scene, 32768)", "show('set_wavefront')", "launch(0)",
          "hip.set_wavefront(scene, 65536)", "show('set_wavefront2')", "launch(0)", "frame(1)", "launch(1)"],
    # hipMalloc refuses the table: the launch evaluates per path, the cache halves until it fits; then hipMalloc refuses more, the pool halves, and the
    # shrunk pool stays for the next frame
    "e": ["frame(0)", "hip.set_transform_table(scene, 1)", "launch(0)", "os.environ['FAKEHIP_MALLOC_MAX'] = str(64 << 20)",
          "hip.set_wavefront(scene, 524288)", "show('set_wavefront')", "launch(0)", "frame(1)", "launch(1)"],
}
ENV = {
    "a": {"TRAYHIP_XF_CACHE_BYTES": str(4 * TR_XF_REC * 4 * 32768)},   # a cache budget of 32 768 lanes for the four moving instances
    "b": {"TRAYHIP_WF_SLOTS": "65536"},
    "c": {"TRAYHIP_WF_SLOTS": "65536"},
    "d": {},
    "e": {"FAKEHIP_MALLOC_MAX": str(1 << 30)},   # (and a 128 x 128 film: 256 tiles, a pool of up to 2^20 slots)
}

# tray_last_schedule after every step: (pool_slots, xf_cache_bytes, xf_table_bytes, transform_table)
TABLE = (1 << 24) * 5 * TR_XF_REC * 4   # the table's buffer: 2^24 time indices x (four moving instances + the camera)
EXPECTED = {
    # (the cache of 32 768 lanes is too small for the 131 072 slots of the pool the table launch left: it is allocated anew for the pool)
    "a": [("frame0", (0, 0, 0, 0)), ("launch0", (32768, 16 << 20, 0, 0)), ("set_wavefront", (0, 16 << 20, 0, 0)), ("launch0", (131072, 16 << 20, TABLE, 1)),
          ("launch0", (131072, 64 << 20, TABLE, 0))],
    "b": [("frame0", (0, 0, 0, 0)), ("launch0", (65536, 0, TABLE, 1)), ("frame1", (65536, 0, TABLE, 0)), ("launch1", (65536, 0, TABLE, 1)),
          ("frame2", (65536, 0, TABLE, 0)), ("launch2", (65536, 0, TABLE, 1))],
    "c": [("frame0", (0, 0, 0, 0)), ("launch0", (65536, 32 << 20, 0, 0)), ("frame1", (65536, 32 << 20, 0, 0)), ("launch1", (65536, 32 << 20, 0, 0)),
          ("frame2", (65536, 32 << 20, 0, 0)), ("launch2", (65536, 32 << 20, 0, 0))],
    "d": [("frame0", (0, 0, 0, 0)), ("launch0", (262144, 0, TABLE, 1)), ("set_wavefront", (0, 0, TABLE, 1)), ("launch0", (32768, 0, TABLE, 1)),
          ("set_wavefront2", (0, 0, TABLE, 1)), ("launch0", (65536, 0, TABLE, 1)), ("frame1", (65536, 0, TABLE, 0)), ("launch1", (65536, 0, TABLE, 1))],
    "e": [("frame0", (0, 0, 0, 0)), ("launch0", (1 << 20, 512 << 20, 0, 0)), ("set_wavefront", (0, 512 << 20, 0, 0)), ("launch0", (131072, 512 << 20, 0, 0)),
          ("frame1", (131072, 512 << 20, 0, 0)), ("launch1", (131072, 512 << 20, 0, 0))],
}

