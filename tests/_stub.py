"""The stand-in runtimes of the stub tests (tests/stubs/fakehip.c, preloaded in place of the HIP runtime; tests/stubs/fakerccl.c, the dlopen
target "librccl.so"): built once per session, a driver script run under them in a fresh child process, and the parsers of fakehip.c's log.
Test infrastructure only; a test module imports the fixture it needs (`stub`, or `stub_rccl` for the multi-device path) and the parsers."""
import functools
import os
import subprocess
import sys

import pytest

STUBS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "stubs")
_built = {}   # library file name -> path (the fixtures below are registered once per importing module: the build is shared through this)


def _build(tmp_path_factory, name, source, libs):
    if name not in _built:
        if "dir" not in _built:
            _built["dir"] = str(tmp_path_factory.mktemp("stubs"))
        _built[name] = os.path.join(_built["dir"], name)
        subprocess.run(["gcc", "-O1", "-shared", "-fPIC", "-o", _built[name], os.path.join(STUBS, source)] + libs, check=True)
    return _built[name]


def run(preload, lib_dir, driver_source, tmp_path, **env):
    """driver_source in a fresh child process under the stub runtime, with FAKEHIP_LOG set; env: further variables (None removes one). The stub
    goes in front of whatever LD_PRELOAD already holds. Returns (the completed process, the log's lines)."""
    log = str(tmp_path / "calls.log")
    e = dict(os.environ, FAKEHIP_LOG=log)
    e["LD_PRELOAD"] = ":".join(p for p in (preload, os.environ.get("LD_PRELOAD", "")) if p)
    if lib_dir:
        e["LD_LIBRARY_PATH"] = lib_dir + ":" + os.environ.get("LD_LIBRARY_PATH", "")
    for k, v in env.items():
        if v is None:
            e.pop(k, None)
        else:
            e[k] = str(v)
    out = subprocess.run([sys.executable, "-c", driver_source], env=e, capture_output=True, text=True, timeout=300)
    return out, open(log).read().splitlines() if os.path.exists(log) else []


@pytest.fixture(scope="session")
def stub(tmp_path_factory, built):
    """run(driver_source, tmp_path, **env) under the stand-in HIP runtime"""
    return functools.partial(run, _build(tmp_path_factory, "libfakehip.so", "fakehip.c", ["-lpthread", "-ldl"]), None)


@pytest.fixture(scope="session")
def stub_rccl(tmp_path_factory, built):
    """the same with the stand-in RCCL on the library path"""
    hip = _build(tmp_path_factory, "libfakehip.so", "fakehip.c", ["-lpthread", "-ldl"])
    return functools.partial(run, hip, os.path.dirname(_build(tmp_path_factory, "librccl.so", "fakerccl.c", ["-ldl"])))


def kv(line):
    """the key=value pairs of a log line"""
    return dict(p.split("=", 1) for p in line.split()[1:])


def tile_launches(log):
    """(range line, launch line) pairs of the tile-kernel launches, in order: a launch's own line is the next launch line of the same device
    (the devices' host threads log side by side)"""
    out = []
    for i, l in enumerate(log):
        if l.startswith("range"):
            r = kv(l)
            out.append((r, next(kv(m) for m in log[i + 1:] if m.startswith("launch") and kv(m)["dev"] == r["dev"])))
    return out


def _template_arg(sym):
    """k_dn_filter<3> is _ZN10tr_denoise11k_dn_filterILi3EEEv...: 3, or -1 without a template argument"""
    return int(sym.split("ILi", 1)[1].split("E", 1)[0]) if "ILi" in sym else -1


def events(log):
    """every launch in order: ("range", begin, end, tile_count, spp, chunk, chunk_stride) per tile kernel, ("noise", kernel, grid, block) per kernel
    of libtrayhip_noise.so, ("denoise", kernel, template argument, grid, block, stream) and ("guide", kernel, template argument or -1, grid, block,
    stream) per kernel of libtrayhip_denoise.so and libtrayhip_guide.so"""
    ranges = iter(tile_launches(log))
    out = []
    for l in log:
        n = kv(l) if l.startswith(("noise", "denoise", "guide")) else None
        if l.startswith("range"):
            r, launch = next(ranges)
            out.append(("range", int(r["begin"]), int(r["end"]), int(launch["tile_count"]), int(launch["spp"]), int(launch["chunk"]),
                        int(launch["chunk_stride"])))
        elif l.startswith("noise"):
            out.append(("noise", next((k for k in ("compact", "error") if k in n["kernel"]), n["kernel"]), int(n["grid"]), int(n["block"])))
        elif l.startswith("denoise"):
            sym = n["kernel"]
            name = "prepare" if "k_dn_prepare" in sym else "filter" if "k_dn_filter" in sym else sym
            out.append(("denoise", name, _template_arg(sym), int(n["grid"]), int(n["block"]), n["stream"]))
        elif l.startswith("guide"):
            sym = n["kernel"]
            name = next((k for k in ("k_dn_filter_halves", "k_guide_mark", "k_guide_compact") if k in sym), sym)
            out.append(("guide", name, _template_arg(sym), int(n["grid"]), int(n["block"]), n["stream"]))
    return out
