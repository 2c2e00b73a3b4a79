"""The Python front end (tray_rust_amd/__init__.py, class Hip) as a transcript: every call into the C library with its arguments, every
allocation, zero_() and synchronize(), every refusal's type and text, what is printed and what comes back, for every denoiser and render entry
point with its defaults and each option once. No library is built or loaded: tests/_fake_torch.py stands in for torch, a recording object for
the C library (the name `lib` of the package is replaced) and a duck-typed object for the scene. Tensors and host buffers appear by a small
running number or a name, never by an address. One more set of cases wraps the five private methods the GPU tests replace on an instance
(and the two public range renders) and records the order and the shapes they are called with.

The expected transcript, tests/golden/front_end_calls.json.gz (300 KB of JSON, one list of events per case; `zcat` shows it), is a record of what the code did BEFORE the front end was folded into one filter call,
one film intake and one sequence loop; `python tests/test_front_end_calls.py --record` writes it and is not to be run to make a change pass."""
import contextlib
import ctypes as C
import gzip
import io
import json
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:   # (for the recording entry point; under pytest conftest.py has done it)
    sys.path.insert(0, ROOT)

import _fake_torch as FT
import tray_rust_amd as T
from tray_rust_amd import _lib as L

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "front_end_calls.json.gz")
W, H = 16, 8
DEV, STREAM = 0xD0D0, FT.Stream.cuda_stream
SCRATCH_BYTES = 4096


def address(names, value):
    """an address as the name it was given, or as the running number of the tensor that lives there"""
    if value is None or value in names:
        return names.get(value)
    n = FT.number(value)
    return {"address": "unknown"} if n is None else {"t": n}


class Lib:
    """every tray_* name is a function that appends [name, arguments] to the events and answers TRAY_OK"""

    def __init__(self, events, names, timing):
        self.events, self.names, self.timing = events, names, timing

    def show(self, a):
        if a is None or isinstance(a, float):
            return a
        if isinstance(a, int):
            return self.address(a) if a > 1 << 20 else a
        if isinstance(a, C.c_void_p):
            return self.address(a.value)
        if isinstance(a, C.Array):
            return [self.address(v) for v in a] if a._type_ is C.c_void_p else {"array": a._type_.__name__, "length": len(a)}
        if isinstance(a, C._Pointer):
            return {"pointer": type(a).__name__}
        if type(a).__name__ == "CArgObject":   # C.byref(x)
            return {"byref": type(a._obj).__name__}
        return {"object": type(a).__name__}

    def address(self, value):
        return address(self.names, value)

    def __getattr__(self, name):
        if not name.startswith("tray_"):
            raise AttributeError(name)

        def call(*args):
            self.events.append([name, [self.show(a) for a in args]])
            if name.endswith("_scratch_bytes"):
                return SCRATCH_BYTES
            if name == "tray_round_spp":
                return 1 << max(int(args[0]) - 1, 0).bit_length()
            if name == "tray_last_error":
                return b""
            if name == "tray_last_timing":
                return L.TRAY_OK if self.timing else L.TRAY_E_INVALID
            if name == "tray_block_queue":   # (w, h, start, count, buffer, capacity, byref(n)): every 8 x 8 tile, or `count` of them
                args[6]._obj.value = args[3] or ((args[0] + 7) // 8) * ((args[1] + 7) // 8)
            return L.TRAY_OK
        return call


class Scene:
    def __init__(self, events):
        self.events = events

    def device_scene(self, frame=0, device=None):
        self.events.append(["scene.device_scene", int(frame), device])
        return C.c_void_p(DEV)

    def flatten(self, frame=0):
        self.events.append(["scene.flatten", int(frame)])
        return types.SimpleNamespace(contents=types.SimpleNamespace(film=types.SimpleNamespace(width=W, height=H)))

    def release_device(self):
        self.events.append(["scene.release_device"])


class Target(T.RenderTarget):
    def add_pixels(self, rgbw):
        self.events.append(["rt.add_pixels", list(np.shape(rgbw))])
        super().add_pixels(rgbw)


class Env:
    """what a case works with: hip, scene, rt, cfg (16 spp, every block of frame 0) and film makers"""

    def __init__(self, monkeypatch, timing):
        self.events = FT.record()
        self.names = {DEV: "dev", STREAM: "stream"}
        monkeypatch.setitem(sys.modules, "torch", FT.fake_torch())
        fake = Lib(self.events, self.names, timing)
        monkeypatch.setattr(T, "lib", lambda: fake)
        self.hip = T.Hip(0, seed=3)
        self.scene = Scene(self.events)
        self.rt = Target(W, H)
        self.rt.events = self.events
        self.names[self.rt.pixels.ctypes.data] = "rt.pixels"
        self.cfg = T.Config("out", "scene.json", 16, 1, T.FrameInfo(4, 1.0, 0, 3), (0, 0))
        self.kept = []

    def film(self, w=W, h=H):
        a = np.ones((h, w, 4), np.float32)
        self.kept.append(a)   # (alive to the end of the case: an address names one film)
        self.names[a.ctypes.data] = f"film {len(self.kept)}"   # (what the caller hands in goes by its own number, so that the order is seen)
        return a

    def pairs(self, n, w=W, h=H):
        return [(self.film(w, h), self.film(w, h)) for _ in range(n)]

    def films(self, n):
        return [self.film() for _ in range(n)]

    def tensor(self, a=None, device="cuda:0"):
        t = FT.Tensor(self.film() if a is None else a)
        t.device = device
        return t

    def tensors(self, x):
        """the same nesting with every numpy film as a tensor"""
        return self.tensor(x) if isinstance(x, np.ndarray) else type(x)(self.tensors(v) for v in x)

    def describe(self, v):
        if isinstance(v, np.ndarray):
            return {"ndarray": list(v.shape), "dtype": v.dtype.name}
        if isinstance(v, FT.Tensor):
            return address(self.names, v.data_ptr())
        if isinstance(v, dict):
            return {k: self.describe(x) for k, x in sorted(v.items())}
        if isinstance(v, (tuple, list)):
            return [self.describe(x) for x in v]
        if isinstance(v, int) and not isinstance(v, bool) and v > 1 << 20:
            return address(self.names, v)
        if v is None or isinstance(v, (bool, int, float, str)):
            return v
        return {"object": type(v).__name__}

    def spy(self, *names):
        """wraps the named methods ON THE INSTANCE, as the GPU tests do: the events then show what each was called with"""
        for name in names:
            def wrapper(*a, _inner=getattr(self.hip, name), _name=name, **kw):
                self.events.append(["seam", _name, self.describe(a)] + ([self.describe(kw)] if kw else []))
                return _inner(*a, **kw)
            setattr(self.hip, name, wrapper)


SEAMS = ("_denoise_device", "_denoise_halves_device", "_denoise_temporal_device", "_denoise_temporal_halves_device",
         "_denoise_temporal_demodulated_halves_device", "render_samples_device", "render_first_hit_device")
SECOND = dict(radius2=3, patch2=0, k2=0.5)
SECOND_T = dict(SECOND, radius_t2=2)
FIRST = dict(radius=4, patch=2, k=0.3)
FIRST_T = dict(FIRST, radius_t=2)
CASES = {}


def case(name, **variants):
    """registers fn(e, **kw) once per variant, as name or name[variant]; without variants once, as it is"""
    def add(fn):
        for tag, kw in (variants or {"": {}}).items():
            key = f"{name}[{tag}]" if tag else name
            assert key not in CASES, key
            CASES[key] = lambda e, fn=fn, kw=kw: fn(e, **kw)
        return fn
    return add


# ---- renders

@case("render")
def _(e):
    return e.hip.render(e.scene, e.rt, e.cfg)


@case("render_device")
def _(e):
    e.hip.render_device(e.scene, 2, (3, 5), 12, e.tensor().data_ptr(), STREAM)


@case("render_samples_device")
def _(e):
    e.hip.render_samples_device(e.scene, 1, (0, 0), 16, (4, 12), e.tensor().data_ptr())


@case("render_first_hit_device")
def _(e):
    e.hip.render_first_hit_device(e.scene, 1, (0, 0), 16, (0, 4), *[e.tensor().data_ptr() for _ in range(3)], STREAM)


@case("render_first_hit", default={}, sample_range=dict(sample_range=(2, 9)))
def _(e, **kw):
    return e.hip.render_first_hit(e.scene, e.cfg, **kw)


@case("render_progressive", three=dict(passes=3), more_than_spp=dict(passes=40), none=dict(passes=0))
def _(e, passes):
    return [(done, rt is e.rt) for done, rt in e.hip.render_progressive(e.scene, e.rt, e.cfg, passes)]


@case("render_noise_target", default={}, min_spp=dict(min_spp=4), filtered=dict(error="filtered"), filtered_parameters=dict(error="filtered", **FIRST),
      max_ratio=dict(max_ratio=4), filtered_max_ratio=dict(error="filtered", max_ratio=2), bad_error=dict(error="both"))
def _(e, **kw):
    return e.hip.render_noise_target(e.scene, e.rt, e.cfg, 0.05, **kw)


@case("render_noise_target[blocks]")
def _(e):
    e.cfg.select_blocks = (1, 1)
    return e.hip.render_noise_target(e.scene, e.rt, e.cfg, 0.05)


@case("render_denoised", default={}, parameters=FIRST, passes2=dict(passes=2), passes2_parameters=dict(passes=2, **SECOND), demodulate=dict(demodulate=True),
      feature_spp=dict(demodulate=True, feature_spp=4), demodulate_passes2=dict(demodulate=True, passes=2), threshold=dict(threshold=0.05),
      threshold_min_spp=dict(threshold=0.05, min_spp=4), threshold_filtered=dict(threshold=0.05, error="filtered", **FIRST),
      threshold_max_ratio=dict(threshold=0.05, max_ratio=4), threshold_filtered_max_ratio=dict(threshold=0.05, error="filtered", max_ratio=4),
      threshold_demodulate_passes2=dict(threshold=0.05, demodulate=True, passes=2),
      bad_error=dict(error="both"), max_ratio_alone=dict(max_ratio=4), passes3=dict(passes=3), filtered_passes2=dict(threshold=0.05, error="filtered", passes=2),
      filtered_demodulate=dict(threshold=0.05, error="filtered", demodulate=True), filtered_alone=dict(error="filtered"),
      feature_spp_0=dict(demodulate=True, feature_spp=0), feature_spp_32=dict(demodulate=True, feature_spp=32))
def _(e, **kw):
    return e.hip.render_denoised(e.scene, e.rt, e.cfg, **kw)


@case("render_denoised[spp1]")
def _(e):
    e.cfg.spp = 1
    return e.hip.render_denoised(e.scene, e.rt, e.cfg)


@case("render_denoised[seams]", default={}, passes2=dict(passes=2), demodulate=dict(demodulate=True, feature_spp=8), threshold=dict(threshold=0.05),
      filtered=dict(threshold=0.05, error="filtered"))
def _(e, **kw):
    e.spy(*SEAMS)
    return e.hip.render_denoised(e.scene, e.rt, e.cfg, **kw)


# ---- the spatial filter calls

@case("denoise", default={}, parameters=FIRST, passes1=dict(passes=1), passes2=dict(passes=2), passes2_parameters=dict(passes=2, **SECOND), passes0=dict(passes=0),
      passes3=dict(passes=3))
def _(e, **kw):
    return e.hip.denoise(e.film(), e.film(), **kw)


@case("denoise[albedo]", default={}, passes2=dict(passes=2, **SECOND))
def _(e, **kw):
    return e.hip.denoise(e.film(), e.film(), albedo=e.film(), **kw)


@case("denoise[tensors]", default={}, passes2=dict(passes=2))
def _(e, **kw):
    return e.hip.denoise(e.tensor(), e.tensor(), **kw)


@case("denoise[tensors_albedo]", default={}, passes2=dict(passes=2))
def _(e, **kw):
    return e.hip.denoise(e.tensor(), e.tensor(), albedo=e.tensor(), **kw)


@case("denoise[one_tensor_twice]")
def _(e):
    t = e.tensor()
    return e.hip.denoise(t, t)


def refused_films(e):
    """name -> (even, odd): pairs no film call takes"""
    return {"mixed": (e.film(), e.tensor()), "other_device": (e.tensor(), e.tensor(device="cuda:1")), "two_dimensions": (e.tensor(np.ones((H, W), np.float32)),) * 2,
            "three_channels": (np.ones((H, W, 3), np.float32),) * 2, "two_sizes": (e.film(), e.film(W + 1))}


REFUSED_FILMS = ("mixed", "other_device", "two_dimensions", "three_channels", "two_sizes")


@case("denoise[refused]", **{n: dict(which=n) for n in REFUSED_FILMS})
def _(e, which):
    return e.hip.denoise(*refused_films(e)[which])


@case("denoise[refused_albedo]", kind=dict(which="kind"), kind_tensors=dict(which="kind_tensors"), size=dict(which="size"), other_device=dict(which="other_device"),
      two_dimensions=dict(which="two_dimensions"), three_channels=dict(which="three_channels"))
def _(e, which):
    if which in ("kind_tensors", "other_device"):
        return e.hip.denoise(e.tensor(), e.tensor(), albedo=e.film() if which == "kind_tensors" else e.tensor(device="cuda:1"))
    albedo = {"kind": lambda: e.tensor(), "size": lambda: e.film(W, H + 1), "two_dimensions": lambda: np.ones((H, W), np.float32),
              "three_channels": lambda: np.ones((H, W, 3), np.float32)}[which]()
    return e.hip.denoise(e.film(), e.film(), albedo=albedo)


@case("denoise_guided", default={}, parameters=FIRST)
def _(e, **kw):
    return e.hip.denoise_guided(e.film(), e.film(), e.film(), e.film(), **kw)


@case("denoise_guided[tensors]", different={}, own_guide=dict(own=True), one_guide_twice=dict(twice=True))
def _(e, own=False, twice=False):
    a, b, g = e.tensor(), e.tensor(), e.tensor()
    return e.hip.denoise_guided(a, b, *((a, b) if own else (g, g) if twice else (g, e.tensor())))


@case("denoise_guided[refused_films]", **{n: dict(which=n) for n in REFUSED_FILMS})
def _(e, which):
    return e.hip.denoise_guided(*refused_films(e)[which], e.film(), e.film())


@case("denoise_guided[refused_guide]", **{n: dict(which=n) for n in REFUSED_FILMS}, kind=dict(which="kind"), size=dict(which="size"))
def _(e, which):
    guide = (e.tensor(), e.tensor()) if which == "kind" else (e.film(W + 2), e.film(W + 2)) if which == "size" else refused_films(e)[which]
    return e.hip.denoise_guided(e.film(), e.film(), *guide)


@case("denoise_halves", default={}, parameters=FIRST)
def _(e, **kw):
    return e.hip.denoise_halves(e.film(), e.film(), **kw)


@case("denoise_halves[tensors]", different={}, one_tensor_twice=dict(twice=True))
def _(e, twice=False):
    t = e.tensor()
    return e.hip.denoise_halves(t, t if twice else e.tensor())


@case("denoise_halves[refused]", **{n: dict(which=n) for n in REFUSED_FILMS})
def _(e, which):
    return e.hip.denoise_halves(*refused_films(e)[which])


# ---- the temporal filter calls: frames (and albedos, and guides) as numpy arrays or as tensors, every centre of three frames and one frame alone

def temporal(e, method, n=3, tensors=False, albedos=False, guides=False, centre=1, **kw):
    """hip.<method>(frames[, albedos][, guides], centre, **kw) of n frames"""
    args = [e.pairs(n)] + ([e.films(n)] if albedos else []) + ([e.pairs(n)] if guides else [])
    return getattr(e.hip, method)(*(e.tensors(args) if tensors else args), centre, **kw)


LISTS = dict(centre0=dict(centre=0), centre1=dict(centre=1), centre2=dict(centre=2), one_frame=dict(n=1, centre=0), tensors=dict(tensors=True),
             tensors_centre2=dict(tensors=True, centre=2), tensors_one_frame=dict(tensors=True, n=1, centre=0), parameters=FIRST_T,
             centre_3=dict(centre=3), centre_negative=dict(centre=-1), no_frame=dict(n=0, centre=0))
TWO = dict(passes1=dict(passes=1), passes2=dict(passes=2), passes2_parameters=dict(passes=2, **SECOND_T), passes2_tensors=dict(passes=2, tensors=True),
           passes2_one_frame=dict(passes=2, n=1, centre=0), passes2_centre0=dict(passes=2, centre=0), passes3=dict(passes=3))


@case("denoise_temporal", **LISTS, **TWO)
def _(e, **kw):
    return temporal(e, "denoise_temporal", **kw)


@case("denoise_temporal[albedos]", default={}, centre0=dict(centre=0), centre2=dict(centre=2), one_frame=dict(n=1, centre=0), tensors=dict(tensors=True),
      parameters=FIRST_T, passes2=dict(passes=2))
def _(e, n=3, tensors=False, centre=1, **kw):
    frames, albedos = e.pairs(n), e.films(n)
    if tensors:
        frames, albedos = e.tensors(frames), e.tensors(albedos)
    return e.hip.denoise_temporal(frames, centre, albedos=albedos, **kw)


@case("denoise_temporal_halves", **LISTS)
def _(e, **kw):
    return temporal(e, "denoise_temporal_halves", **kw)


@case("denoise_temporal_guided", **LISTS)
def _(e, **kw):
    return temporal(e, "denoise_temporal_guided", guides=True, **kw)


@case("denoise_temporal_guided[own_guides]")
def _(e):
    frames = e.tensors(e.pairs(3))
    return e.hip.denoise_temporal_guided(frames, frames, 1)


@case("denoise_temporal_demodulated", **LISTS, **TWO)
def _(e, **kw):
    return temporal(e, "denoise_temporal_demodulated", albedos=True, **kw)


@case("denoise_temporal_demodulated_halves", **LISTS)
def _(e, **kw):
    return temporal(e, "denoise_temporal_demodulated_halves", albedos=True, **kw)


@case("denoise_temporal_demodulated_guided", **LISTS)
def _(e, **kw):
    return temporal(e, "denoise_temporal_demodulated_guided", albedos=True, guides=True, **kw)


def refused_lists(e, which, tensors=False):
    """(frames, albedos, guides) of three frames with one thing wrong"""
    frames, albedos, guides = e.pairs(3), e.films(3), e.pairs(3)
    if tensors:
        frames, albedos, guides = e.tensors(frames), e.tensors(albedos), e.tensors(guides)
    bad = refused_films(e)
    if which.startswith("frame_"):
        frames[2] = bad[which[6:]]
    elif which.startswith("guide_"):
        guides[2] = bad[which[6:]]
    elif which == "frames_kinds":
        frames[2] = e.tensors(frames[2])
    elif which == "frames_sizes":
        frames[0] = (e.film(W, H + 1), e.film(W, H + 1))
    elif which == "fewer_albedos":
        albedos = albedos[:2]
    elif which == "albedos_kinds":
        albedos[1] = e.film() if tensors else e.tensor()
    elif which == "albedo_other_device":
        albedos[1] = e.tensor(device="cuda:1")
    elif which == "albedo_two_dimensions":
        albedos[0] = np.ones((H, W), np.float32)
    elif which == "albedo_three_channels":
        albedos[0] = np.ones((H, W, 3), np.float32)
    elif which == "albedos_size":
        albedos[2] = e.film(W + 1)
    elif which == "fewer_guides":
        guides = guides[:2]
    elif which == "guides_kinds":
        guides = e.pairs(3) if tensors else e.tensors(guides)
    elif which == "guides_mixed":
        guides[0] = e.pairs(1)[0] if tensors else e.tensors(guides[0])
    elif which == "guides_sizes":
        guides[1] = (e.film(W + 1), e.film(W + 1))
    elif which == "guides_size":
        guides = e.pairs(3, W, H + 2)
    else:
        raise KeyError(which)
    return frames, albedos, guides


WRONG_FRAMES = ["frame_" + n for n in REFUSED_FILMS] + ["frames_kinds", "frames_sizes"]
WRONG_ALBEDOS = ["fewer_albedos", "albedos_kinds", "albedo_two_dimensions", "albedo_three_channels", "albedos_size"]
WRONG_GUIDES = ["guide_" + n for n in REFUSED_FILMS] + ["fewer_guides", "guides_kinds", "guides_mixed", "guides_sizes", "guides_size"]
which = lambda names, **kw: {n: dict(which=n, **kw) for n in names}
which_tensors = lambda names: {n + "_tensors": dict(which=n, tensors=True) for n in names}


@case("denoise_temporal[refused]", **which(WRONG_FRAMES + WRONG_ALBEDOS), **which_tensors(["albedos_kinds", "albedo_other_device", "frames_sizes"]),
      passes2_albedos=dict(which="fewer_albedos", passes=2))
def _(e, which, tensors=False, **kw):
    frames, albedos, _ = refused_lists(e, which, tensors)
    return e.hip.denoise_temporal(frames, 1, albedos=albedos if "albedo" in which else None, **kw)


@case("denoise_temporal_halves[refused]", **which(WRONG_FRAMES))
def _(e, which):
    return e.hip.denoise_temporal_halves(refused_lists(e, which)[0], 1)


@case("denoise_temporal_guided[refused]", **which(WRONG_FRAMES + WRONG_GUIDES), **which_tensors(["guides_kinds", "guides_mixed"]))
def _(e, which, tensors=False):
    frames, _, guides = refused_lists(e, which, tensors)
    return e.hip.denoise_temporal_guided(frames, guides, 1)


@case("denoise_temporal_demodulated[refused]", **which(WRONG_FRAMES + WRONG_ALBEDOS), **which_tensors(["albedos_kinds", "albedo_other_device"]))
def _(e, which, tensors=False):
    frames, albedos, _ = refused_lists(e, which, tensors)
    return e.hip.denoise_temporal_demodulated(frames, albedos, 1)


@case("denoise_temporal_demodulated_halves[refused]", **which(WRONG_FRAMES + WRONG_ALBEDOS))
def _(e, which):
    frames, albedos, _ = refused_lists(e, which)
    return e.hip.denoise_temporal_demodulated_halves(frames, albedos, 1)


@case("denoise_temporal_demodulated_guided[refused]", **which(WRONG_FRAMES + WRONG_ALBEDOS + WRONG_GUIDES), **which_tensors(["albedos_kinds", "guides_kinds"]))
def _(e, which, tensors=False):
    return e.hip.denoise_temporal_demodulated_guided(*refused_lists(e, which, tensors), 1)


# ---- the two sequence generators

def sequence(e, method, frames=range(4), seams=False, **kw):
    if seams:
        e.spy(*SEAMS)
    out = []
    for frame, image in getattr(e.hip, method)(e.scene, e.cfg, frames, **kw):
        e.events.append(["yielded", frame, e.describe(image)])
        out.append(frame)
    return out


REACHES = {f"reach{r}": dict(reach=r) for r in (0, 1, 2)}
REFUSED_SEQUENCE = dict(frames_with_a_gap=dict(frames=[0, 1, 3]), frames_descending=dict(frames=[2, 1]), reach5=dict(reach=5), reach_negative=dict(reach=-1),
                        no_frames=dict(frames=[]), passes3=dict(passes=3))


def modes(mode, **more):
    """every reach, once with the seams wrapped at reach 1 and three frames, the parameters once"""
    out = {tag: dict(kw, **mode) for tag, kw in REACHES.items()}
    out["seams"] = dict(mode, seams=True, frames=range(3), reach=1)
    out["default_reach"] = dict(mode)
    out["frames_from_5"] = dict(mode, frames=range(5, 8))
    out["one_frame"] = dict(mode, frames=[2])
    out.update({tag: dict(mode, **kw) for tag, kw in more.items()})
    return out


@case("render_sequence_denoised[plain]", **modes({}, parameters=FIRST_T), **REFUSED_SEQUENCE)
@case("render_sequence_denoised[demodulate]", **modes(dict(demodulate=True), parameters=dict(FIRST_T, feature_spp=4), feature_spp_0=dict(feature_spp=0),
                                                      feature_spp_32=dict(feature_spp=32)))
@case("render_sequence_denoised[passes2]", **modes(dict(passes=2), parameters=dict(FIRST_T, **SECOND_T), demodulate=dict(demodulate=True)))
def _(e, **kw):
    return sequence(e, "render_sequence_denoised", **kw)


@case("render_sequence_denoised[spp1]", plain={}, demodulate=dict(demodulate=True))
def _(e, **kw):
    e.cfg.spp = 1
    return sequence(e, "render_sequence_denoised", **kw)


@case("render_sequence_demodulated[passes2]", **modes({}, parameters=dict(FIRST_T, feature_spp=4, **SECOND_T), feature_spp_0=dict(feature_spp=0),
                                                       feature_spp_32=dict(feature_spp=32)), **REFUSED_SEQUENCE)
@case("render_sequence_demodulated[passes1]", **modes(dict(passes=1), parameters=dict(FIRST_T, feature_spp=4), feature_spp_0=dict(feature_spp=0)),
      **{k: dict(v, passes=1) for k, v in REFUSED_SEQUENCE.items() if k != "passes3"})
def _(e, **kw):
    return sequence(e, "render_sequence_demodulated", **kw)


@case("render_sequence_demodulated[spp1]")
def _(e):
    e.cfg.spp = 1
    return sequence(e, "render_sequence_demodulated")


def transcript(name, timing):
    """the events of one case with tray_last_timing answering (timing) or refusing"""
    with pytest.MonkeyPatch.context() as monkeypatch:
        e = Env(monkeypatch, timing)
        printed = io.StringIO()
        with contextlib.redirect_stdout(printed):
            try:
                result = ["returned", e.describe(CASES[name](e))]
            except (ValueError, TypeError, T.TrayError) as error:
                result = ["raised", type(error).__name__, str(error)]
        if printed.getvalue():
            e.events.append(["printed", printed.getvalue()])
        e.events.append(result)
        return json.loads(json.dumps(e.events))   # (as the stored one: tuples are lists)


def timings(name, index):
    """tray_last_timing answers in every other case; the four methods that ask it are seen both ways"""
    both = name.split("[")[0] in ("render", "render_progressive", "render_noise_target", "render_denoised") and "seams" not in name
    return (True, False) if both else (index % 2 == 0,)


RUNS = [(name, timing) for index, name in enumerate(CASES) for timing in timings(name, index)]
key = lambda name, timing: f"{name} timing={'yes' if timing else 'no'}"


@pytest.fixture(scope="module")
def golden():
    with gzip.open(GOLDEN, "rt") as f:
        return json.load(f)


def test_the_record_holds_these_cases_and_no_others(golden):
    assert sorted(golden) == sorted(key(*run) for run in RUNS)


GROUPS = sorted({name.split("[")[0] for name in CASES})   # one test per entry point: the cases are quick, a test item each is not


@pytest.mark.parametrize("group", GROUPS)
def test_front_end_transcript(golden, group):
    for name, timing in RUNS:
        if name.split("[")[0] == group:
            got, want = transcript(name, timing), golden[key(name, timing)]
            for i, (g, w) in enumerate(zip(got, want)):
                assert g == w, f"{key(name, timing)}, event {i} of {len(want)}: {g} instead of {w}"
            assert len(got) == len(want), (key(name, timing), got[len(want):], want[len(got):])


def test_the_seams_see_what_the_gpu_tests_rely_on(golden):
    """the table of the five seams, read off the record: these are the facts the spies of tests/test_gpu_*.py assert on a device"""
    seams = lambda k: [ev[1:] for ev in golden[k] if ev[0] == "seam"]
    # render_sequence_demodulated over three frames at reach 1: a frame's own halves with no neighbours, then the centre's with its window
    td = [args for name, args, *_ in seams("render_sequence_demodulated[passes2][seams] timing=" + timing_of("render_sequence_demodulated[passes2][seams]"))
          if name == "_denoise_temporal_demodulated_halves_device"]
    assert [1 + len(a[1]) for a in td] == [1, 1, 2, 1, 3, 2]
    # render_sequence_denoised(passes=2): every frame's own halves once, through _denoise_halves_device, films first; the pilots' windows
    t2 = seams("render_sequence_denoised[passes2][seams] timing=" + timing_of("render_sequence_denoised[passes2][seams]"))
    own = [args[0]["t"] for name, args, *_ in t2 if name == "_denoise_halves_device"]
    assert len(own) == 3 and len(set(own)) == 3
    assert [1 + len(args[1]) for name, args, *_ in t2 if name == "_denoise_temporal_halves_device"] == [2, 3, 2]
    # plain and demodulate=True: every frame through _denoise_temporal_device, the albedos as the seventh positional argument
    for mode, n_args in (("plain", 6), ("demodulate", 7)):
        k = f"render_sequence_denoised[{mode}][seams]"
        calls = [args for name, args, *_ in seams(f"{k} timing={timing_of(k)}") if name == "_denoise_temporal_device"]
        assert [1 + len(a[1]) for a in calls] == [2, 3, 2] and all(len(a) == n_args for a in calls)
    # render_denoised filters through _denoise_device
    for mode in ("default", "passes2", "demodulate", "threshold"):
        k = f"render_denoised[seams][{mode}]"
        assert sum(name == "_denoise_device" for name, *_ in seams(f"{k} timing={timing_of(k)}")) == 1


def timing_of(name):
    (timing,) = [t for n, t in RUNS if n == name]
    return "yes" if timing else "no"


if __name__ == "__main__":
    assert sys.argv[1:] == ["--record"], "usage: python tests/test_front_end_calls.py --record"
    text = json.dumps({key(*run): transcript(*run) for run in RUNS}, separators=(",", ":"), sort_keys=True) + "\n"
    with open(GOLDEN, "wb") as f:
        f.write(gzip.compress(text.encode(), 9, mtime=0))   # (mtime=0: the same transcripts give the same file)
    print(f"{len(RUNS)} transcripts written to {GOLDEN}")
