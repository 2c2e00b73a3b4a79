#!/usr/bin/env python3
"""The host-side footprint of small wavefront launches of a build of libtrayhip.so under the stand-in HIP runtime (tests/stubs/fakehip.c, with
FAKEHIP_LOG_MEM): every allocation's size, every memset and every kernel launch (symbol, grid, block, dynamic LDS, stream), for a static and a moving
scene x one and two views x TRAYHIP_WF_FUSED 0 / 1 x TRAYHIP_WF_BIN 0 / 3. Pointers are rewritten so that two runs compare line for line: one inside
an allocation as A<allocation's number>+<offset>, any other (streams, host memory) as P<order of first appearance>. No GPU.
    tools/wf_stub_logs.py OUT [path/to/libtrayhip.so]        then `diff` the OUT files of two builds (profiles/r21_wavefront_plan.txt)"""
import itertools
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DRIVER = r'''
import sys
sys.path.insert(0, %(root)r)
import tray_rust_amd as T
scene, rt, spp, fi = T.Scene.load_file(%(path)r)
hip = T.Hip(0, seed=4)
hip.render(scene, rt, T.Config(".", "s", spp, 1, fi, (0, 0)))
print("schedule", sorted(hip.schedule(scene).items()), "timing", hip.timing(scene).launches)
'''


def normalise(lines):
    allocs, others, out = [], {}, []

    def name(m):
        p = int(m.group(0), 16)
        for i, (base, size) in enumerate(allocs):
            if base <= p < base + max(size, 1):
                return "A%d+%d" % (i, p - base)
        return "P%d" % others.setdefault(p, len(others))

    for l in lines:
        if l.startswith("malloc "):
            allocs.append((int(l.split("ptr=")[1], 16), int(l.split("bytes=")[1].split()[0])))
        out.append(re.sub(r"0x[0-9a-f]+", name, l))
    return out


def main(out_path, lib=None):
    from tray_rust_amd import scenes
    with tempfile.TemporaryDirectory() as d:
        stub = os.path.join(d, "libfakehip.so")
        subprocess.run(["gcc", "-O1", "-shared", "-fPIC", "-o", stub, os.path.join(ROOT, "tests", "stubs", "fakehip.c"), "-lpthread", "-ldl"], check=True)
        scenes.write_assets(d, cornell=(128, 128, 16))   # 256 tiles: 256 chunks in use, enough for two views
        paths = {"static": os.path.join(d, "cornell_box.json"), "moving": scenes.write_moving_box(d, width=128, height=128, samples=16)}
        with open(out_path, "w") as out:
            for scene, views, fused, bins in itertools.product(("static", "moving"), (1, 2), (0, 1), (0, 3)):
                log = os.path.join(d, "calls.log")
                if os.path.exists(log):
                    os.remove(log)
                env = dict(os.environ, LD_PRELOAD=stub, FAKEHIP_LOG=log, FAKEHIP_LOG_MEM="1", FAKEHIP_DEVICES="1", FAKEHIP_WF_DONE="1", FAKEHIP_FREE_BYTES=str(4 << 30),
                           TRAYHIP_MODE="wave", TRAYHIP_WF_SLOTS="65536", TRAYHIP_WF_PIPES=str(views), TRAYHIP_WF_FUSED=str(fused), TRAYHIP_WF_BIN=str(bins))
                if lib:
                    env["TRAYHIP_LIB"] = os.path.abspath(lib)
                run = subprocess.run([sys.executable, "-c", DRIVER % {"root": ROOT, "path": paths[scene]}], env=env, capture_output=True, text=True, timeout=300)
                if run.returncode != 0 or "schedule" not in run.stdout:
                    sys.exit("the driver failed: " + run.stdout + run.stderr)
                lines = normalise(open(log).read().splitlines())
                out.write("== %s scene, %d view(s), TRAYHIP_WF_FUSED=%d, TRAYHIP_WF_BIN=%d: %d lines\n" % (scene, views, fused, bins, len(lines)))
                out.write(run.stdout.strip() + "\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main(*sys.argv[1:3])
