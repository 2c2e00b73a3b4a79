"""tray_rust_amd — MI355X-native tile worker for tray_rust scenes.

Host-side mirror of the reference's interface for the hot path (names, argument meaning and error
behaviour follow /root/reference):

    Scene.load_file(path) -> (scene, rt, spp, frame_info)      src/scene.rs:101-145
    FrameInfo, Config                                           src/film/mod.rs:19-36, src/exec/mod.rs:17-38
    Hip().render(scene, rt, config)                             trait Exec, src/exec/mod.rs:41-49
    RenderTarget.get_renderf32 / get_render / clear             src/film/render_target.rs:168-266
    RenderTarget.get_rendered_blocks / add_blocks               src/film/render_target.rs:215-241, src/film/image.rs:36-50
    distrib.worker_node(Hip()) / `python -m tray_rust_amd --worker`   src/exec/distrib/worker.rs, src/main.rs:148-166
    BlockQueue(img, dim, select_blocks)                         src/sampler/block_queue.rs:11-66
    sampler.LowDiscrepancy / Uniform / Adaptive                 src/sampler/{ld,uniform,adaptive}.rs (Hip(sampler=...))

Everything below the Python layer is libtrayhip.so (include/trayhip.h): a C++ scene loader and
hand-written HIP kernels for gfx950. The reference panics on invalid input; here the same
preconditions raise TrayError. There is no CPU fallback: without the library / a GPU the calls fail.
"""
import ctypes as C
import os

import numpy as np

from . import _lib
from . import sampler
from ._lib import TrayError, lib, check

__all__ = ["Scene", "FrameInfo", "Config", "RenderTarget", "Hip", "BlockQueue", "TrayError", "round_spp", "sampler"]


def round_spp(spp):
    """LowDiscrepancy::new rounds spp up to a power of two (src/sampler/ld.rs:22-25)."""
    r = int(lib().tray_round_spp(int(spp)))
    if r != spp:
        print(f"Warning: LowDiscrepancy sampler requires power of two samples per pixel, rounding up to {r}")
    return r


class FrameInfo:
    """src/film/mod.rs:19-36"""

    def __init__(self, frames, time, start, end):
        self.frames, self.time, self.start, self.end = int(frames), float(time), int(start), int(end)

    def __repr__(self):
        return f"FrameInfo(frames={self.frames}, time={self.time}, start={self.start}, end={self.end})"


class Config:
    """src/exec/mod.rs:17-38; select_blocks = (start, count) into the Morton tile queue, count 0 = all."""

    def __init__(self, out_path, scene_file, spp, num_threads, frame_info, select_blocks=(0, 0)):
        self.out_path, self.scene_file, self.spp, self.num_threads = out_path, scene_file, int(spp), int(num_threads)
        self.frame_info, self.current_frame, self.select_blocks = frame_info, frame_info.start, tuple(select_blocks)


class BlockQueue:
    """src/sampler/block_queue.rs:28-48: 8x8 tiles in Morton order, optional (start, count) sub-range."""

    def __init__(self, img, dim=(8, 8), select_blocks=(0, 0)):
        if tuple(dim) != (8, 8):
            raise TrayError(_lib.TRAY_E_UNSUPPORTED, "only (8, 8) blocks are supported (exec/multithreaded.rs:32)")
        n = C.c_uint32(0)
        check(lib().tray_block_queue(img[0], img[1], select_blocks[0], select_blocks[1], None, 0, C.byref(n)))
        buf = (C.c_uint32 * (2 * n.value))()
        check(lib().tray_block_queue(img[0], img[1], select_blocks[0], select_blocks[1], buf, n.value, C.byref(n)))
        self.blocks = [(buf[2 * i], buf[2 * i + 1]) for i in range(n.value)]
        self.dimensions = (8, 8)
        if not self.blocks:
            print("Warning: This block queue is empty!")

    def block_dim(self):
        return self.dimensions

    def __len__(self):
        return len(self.blocks)

    def __iter__(self):
        return iter(self.blocks)


class RenderTarget:
    """Accumulated RGBW f32 film in the layout of RenderTarget::get_renderf32
    (src/film/render_target.rs:243-266). The GPU accumulates on the device; this host object merges
    results by addition like film::Image::add_pixels (src/film/image.rs:21-34)."""

    def __init__(self, width, height):
        self.width, self.height = int(width), int(height)
        self.pixels = np.zeros(self.width * self.height * 4, dtype=np.float32)

    def dimensions(self):
        return (self.width, self.height)

    def clear(self):
        self.pixels[:] = 0.0

    def add_pixels(self, rgbw):
        self.pixels += np.asarray(rgbw, dtype=np.float32).reshape(-1)

    def get_renderf32(self):
        return self.pixels.copy()

    lock_size = (2, 2)   # the reference's lock blocks, hard-coded by its loader (scene.rs:224)

    def get_rendered_blocks(self):
        """render_target.rs:215-241: (block size, positions in pixels of the 2x2 blocks whose FOUR pixels all have a non-zero
        weight, their RGBW one block after the other) -- what a distributed worker sends to the master. Blocks in row order,
        pixels row-major inside a block. (A block with an untouched pixel is left out whole, as in the reference.)"""
        bw, bh = self.lock_size
        xb, yb = self.width // bw, self.height // bh
        img = self.pixels.reshape(self.height, self.width, 4)[:yb * bh, :xb * bw]
        tiles = img.reshape(yb, bh, xb, bw, 4).transpose(0, 2, 1, 3, 4)          # [by][bx][y][x][rgbw]
        full = (tiles[..., 3] != 0.0).all(axis=(2, 3))
        by, bx = np.nonzero(full)
        blocks = np.stack([bx * bw, by * bh], axis=1).astype(np.uint64)
        return (bw, bh), blocks, np.ascontiguousarray(tiles[by, bx]).reshape(-1)

    def add_blocks(self, block_size, blocks, pixels):
        """film::Image::add_blocks (src/film/image.rs:36-50): what the master does with a worker's blocks"""
        bw, bh = int(block_size[0]), int(block_size[1])
        img = self.pixels.reshape(self.height, self.width, 4)
        px = np.asarray(pixels, dtype=np.float32).reshape(-1, bh, bw, 4)
        for k, (x, y) in enumerate(np.asarray(blocks, dtype=np.int64).reshape(-1, 2)):
            img[y:y + bh, x:x + bw] += px[k]

    def get_render(self):
        """sRGB8, 3 bytes per pixel (render_target.rs:185-210)."""
        out = np.zeros(self.width * self.height * 3, dtype=np.uint8)
        check(lib().tray_resolve_srgb8(self.pixels.ctypes.data, self.width, self.height, out.ctypes.data))
        return out


class Scene:
    """Loaded scene (host side) + its device copy for the current frame."""

    def __init__(self, handle):
        self._h = handle
        self._dev = None
        self._dev_frame = None
        self._dev_device = None
        info = _lib.TraySceneInfo()
        check(lib().tray_host_scene_info(self._h, C.byref(info)))
        self.info = info

    @staticmethod
    def load_file(path):
        """Scene::load_file -> (scene, render_target, spp, frame_info)"""
        h = C.c_void_p()
        check(lib().tray_scene_load_file(os.fsencode(path), C.byref(h)))
        return Scene._finish(h)

    @staticmethod
    def load_string(text, base_dir=""):
        h = C.c_void_p()
        check(lib().tray_scene_load_string(text.encode("utf-8"), os.fsencode(base_dir), C.byref(h)))
        return Scene._finish(h)

    @staticmethod
    def _finish(h):
        s = Scene(h)
        i = s.info
        return s, RenderTarget(i.width, i.height), int(i.spp), FrameInfo(i.frames, i.scene_time, i.start_frame, i.end_frame)

    def flatten(self, frame=0):
        """Scene::update_frame + lowering to the TrayFlatScene POD. The view borrows from this scene -- it is valid until the next
        flatten() / close() -- so the returned pointer keeps the scene alive (`T.Scene.load_file(p)[0].flatten(0)` must not dangle)."""
        p = C.POINTER(_lib.TrayFlatScene)()
        check(lib().tray_host_scene_flatten(self._h, int(frame), C.byref(p)))
        p._scene = self
        return p

    def device_scene(self, frame=0, device=None):
        if self._dev is not None and device is not None and device != self._dev_device:
            self.release_device()
        if self._dev is not None and self._dev_frame != frame:
            # Scene::update_frame (scene.rs:152-176): the device copy moves to the new frame, meshes / tables / pools stay where they are
            try:
                check(lib().tray_scene_update_frame(self._dev, self.flatten(frame)))
            except TrayError:
                self.release_device()   # a failed update leaves a handle that can only be destroyed
                raise
            self._dev_frame = frame
        if self._dev is None:
            flat = self.flatten(frame)   # host work first: a scene that cannot be flattened fails here, with or without a GPU
            if device is not None:
                check(lib().tray_init(int(device)))
            d = C.c_void_p()
            check(lib().tray_scene_create(flat, C.byref(d)))
            self._dev, self._dev_frame, self._dev_device = d, frame, device
        return self._dev

    def release_device(self):
        if self._dev is not None:
            lib().tray_scene_destroy(self._dev)
            self._dev = None

    def close(self):
        self.release_device()
        if self._h is not None:
            lib().tray_host_scene_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# the nouns of the film intake's refusals (Hip._films_on_device): of the calls that take lists of frames, and of those that take one frame's films
_FRAMES = {"frames": "frames", "albedo": "albedo films", "guides": "guides", "film": "a film must be (h, w, 4)", "albedo_kind_first": True}
_FILMS = {"frames": "films", "albedo": "albedo film", "guides": "guide", "film": "even and odd must be two (h, w, 4) films of one size",
          "albedo_kind_first": False}   # (albedo_kind_first: an albedo film of the wrong kind is refused before it is looked at, or after)


def _ptr(tensor):
    return C.c_void_p(tensor.data_ptr())


def _current_stream():
    """torch's current stream as the C calls take it"""
    import torch
    stream = torch.cuda.current_stream().cuda_stream
    return C.c_void_p(stream) if stream else None


def _scratch(nbytes, device):
    """a call's scratch buffer (never empty); the caller synchronises before it lets go of it"""
    import torch
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


def _as_given(as_numpy, out):
    """a tensor, or a tuple of them, as the kind the caller handed in"""
    if isinstance(out, tuple):
        return tuple(_as_given(as_numpy, t) for t in out)
    return out.cpu().numpy() if as_numpy else out


_PARTITIONS = {"tiles": _lib.TRAY_PARTITION_TILES, "samples": _lib.TRAY_PARTITION_SAMPLES}   # tray_multi_set_partition


class Hip:
    """Execution backend in the place of exec::MultiThreaded (src/exec/multithreaded.rs:20-70): renders
    config.select_blocks of frame config.current_frame on one MI355X and adds the result into rt."""

    def __init__(self, device=0, seed=1, sampler=None):
        """sampler: callable (block_dim, spp) -> sampler.LowDiscrepancy / Uniform / Adaptive -- what thread_work constructs per worker
        (exec/multithreaded.rs:74); None = LowDiscrepancy::new(block_dim, spp)."""
        self.device, self.seed = int(device), int(seed)
        self.sampler = sampler
        check(lib().tray_init(self.device))
        self.last_timing = None
        self._multi, self._multi_key, self._multi_frame, self._multi_scene = None, None, None, None

    def _select_sampler(self, dev, spp, multi=False):
        """tells the device scene which Sampler the next render stands for; returns the spp the render call takes"""
        if self.sampler is None:
            smp_kind, lo, hi, spp = sampler.LOW_DISCREPANCY, 1, 1, round_spp(spp)
        else:
            smp = self.sampler((8, 8), spp)     # BlockQueue::block_dim (main.rs:101: (8, 8))
            smp_kind, lo, hi, spp = smp.KIND, smp.min_spp, smp.max_spp_, smp.spp
        check((lib().tray_multi_set_sampler if multi else lib().tray_scene_set_sampler)(dev, smp_kind, lo, hi))
        return spp

    def render(self, scene, rt, config):
        dev = scene.device_scene(config.current_frame, self.device)
        spp = self._select_sampler(dev, config.spp)
        start, count = config.select_blocks
        check(lib().tray_render_tiles(dev, int(start), int(count), spp, self.seed, rt.pixels.ctypes.data))
        t = self._keep_timing(dev)
        if t is not None:
            print(f"Frame {config.current_frame}: rendering took {t.render_ms * 1e-3:.4f}s")

    def render_device(self, scene, frame, select_blocks, spp, rgbw_ptr, stream=None):
        """Asynchronous variant: accumulate into a device RGBW buffer (e.g. torch tensor .data_ptr())."""
        dev = scene.device_scene(frame, self.device)
        spp = self._select_sampler(dev, spp)
        check(lib().tray_render_tiles_device(dev, int(select_blocks[0]), int(select_blocks[1]), int(spp), self.seed,
                                             C.c_void_p(int(rgbw_ptr)), C.c_void_p(int(stream)) if stream else None))
        return dev

    def render_samples_device(self, scene, frame, select_blocks, spp, sample_range, rgbw_ptr, stream=None):
        """Asynchronous: the samples [begin, end) = sample_range of every pixel of select_blocks of the spp-sample LowDiscrepancy frame,
        accumulated into a device RGBW buffer (tray_render_samples_device). Ranges that partition [0, spp) add up to render_device's film."""
        dev = scene.device_scene(frame, self.device)
        spp = self._select_sampler(dev, spp)
        begin, end = (int(v) for v in sample_range)
        check(lib().tray_render_samples_device(dev, int(select_blocks[0]), int(select_blocks[1]), int(spp), begin, end, self.seed,
                                               C.c_void_p(int(rgbw_ptr)), C.c_void_p(int(stream)) if stream else None))
        return dev

    def render_first_hit_device(self, scene, frame, select_blocks, spp, sample_range, albedo_ptr, normal_ptr, depth_ptr, stream=None):
        """Asynchronous: the first-hit feature films of the samples [begin, end) = sample_range of every pixel of select_blocks of the spp-sample
        LowDiscrepancy frame -- the camera rays render_samples_device traces for them --, accumulated into three device RGBW buffers: albedo,
        shading normal, depth as (distance, coverage, 0) (tray_render_first_hit_device). Ranges add up, weight for weight with the colour film."""
        dev = scene.device_scene(frame, self.device)
        spp = self._select_sampler(dev, spp)
        begin, end = (int(v) for v in sample_range)
        check(lib().tray_render_first_hit_device(dev, int(select_blocks[0]), int(select_blocks[1]), int(spp), begin, end, self.seed,
                                                 C.c_void_p(int(albedo_ptr)), C.c_void_p(int(normal_ptr)), C.c_void_p(int(depth_ptr)),
                                                 C.c_void_p(int(stream)) if stream else None))
        return dev

    def render_first_hit(self, scene, config, sample_range=None):
        """The first-hit films of config.select_blocks of the frame as a dict of three (h, w, 4) numpy RGBW films, "albedo", "normal" and "depth"
        (render_first_hit_device), of the samples sample_range (default: all) of the round_spp(config.spp)-sample frame."""
        import torch
        flat = scene.flatten(config.current_frame).contents.film
        w, h = int(flat.width), int(flat.height)
        spp = round_spp(config.spp)
        with torch.cuda.device(self.device):
            films = [torch.zeros((h, w, 4), dtype=torch.float32, device=f"cuda:{self.device}") for _ in range(3)]
            stream = torch.cuda.current_stream().cuda_stream
            self.render_first_hit_device(scene, config.current_frame, config.select_blocks, spp, sample_range or (0, spp),
                                         *[f.data_ptr() for f in films], stream or None)
            torch.cuda.current_stream().synchronize()
            return {name: f.cpu().numpy() for name, f in zip(("albedo", "normal", "depth"), films)}

    def render_progressive(self, scene, rt, config, passes):
        """Generator: config.select_blocks of the frame in `passes` consecutive sample ranges of nearly equal size ([k spp / passes,
        (k + 1) spp / passes), at most spp of them), each added into rt as it is done; yields (samples_done, rt) after every pass. After the
        last one rt holds what render() adds. LowDiscrepancy only (TrayError TRAY_E_UNSUPPORTED otherwise)."""
        import torch
        if int(passes) < 1:
            raise ValueError("render_progressive: passes must be >= 1")
        dev = scene.device_scene(config.current_frame, self.device)
        spp = self._select_sampler(dev, config.spp)
        passes = min(int(passes), spp)
        w, h = rt.dimensions()
        with torch.cuda.device(self.device):
            film = torch.empty(h * w * 4, dtype=torch.float32, device=f"cuda:{self.device}")
            stream = torch.cuda.current_stream().cuda_stream
            for k in range(passes):
                begin, end = k * spp // passes, (k + 1) * spp // passes
                film.zero_()
                self.render_samples_device(scene, config.current_frame, config.select_blocks, spp, (begin, end), film.data_ptr(), stream or None)
                rt.add_pixels(film.cpu().numpy())
                self._keep_timing(dev)
                yield end, rt

    def _keep_timing(self, dev):
        """the timing of the device scene's last render call, kept as self.last_timing; None, and nothing kept, where the library has none"""
        t = _lib.TrayKernelTiming()
        if lib().tray_last_timing(dev, C.byref(t)) != _lib.TRAY_OK:
            return None
        self.last_timing = t
        return t

    def _noise_target_device(self, dev, start, count, min_spp, spp, threshold, even, odd, n, error, radius, patch, k, want_out, max_ratio=None):
        """one noise-target call on the current stream into the zeroed (h, w, 4) tensors even / odd: error="raw" is
        tray_render_noise_target_device, "filtered" tray_render_noise_target_filtered_device (with its denoised output if want_out). max_ratio:
        tray_scene_set_noise_ratio for this call alone (the device scene is back at 0 afterwards). Returns (tile_samples, tile_error, out tensor
        or None)."""
        import torch
        if max_ratio is not None:
            check(lib().tray_scene_set_noise_ratio(dev, int(max_ratio)))
        try:
            samples, err = np.zeros(n, np.uint32), np.zeros(n, np.float32)
            head = (dev, start, count, int(min_spp), spp, float(threshold), self.seed, _ptr(even), _ptr(odd))
            tail = (samples.ctypes.data_as(C.POINTER(C.c_uint32)), err.ctypes.data_as(C.POINTER(C.c_float)), _current_stream())
            out = None
            if error == "raw":
                check(lib().tray_render_noise_target_device(*head, *tail))
            else:
                h, w = int(even.shape[0]), int(even.shape[1])
                scratch = _scratch(lib().tray_noise_target_filtered_scratch_bytes(w, h), even.device)
                out = torch.empty_like(even) if want_out else None
                check(lib().tray_render_noise_target_filtered_device(*head, int(radius), int(patch), float(k), _ptr(out) if want_out else None,
                                                                     _ptr(scratch), *tail))
                torch.cuda.current_stream().synchronize()   # (scratch goes out of scope here)
            return samples, err, out
        finally:
            if max_ratio is not None:
                lib().tray_scene_set_noise_ratio(dev, 0)   # (a device scene other methods reuse keeps their behaviour)

    def render_noise_target(self, scene, rt, config, threshold, min_spp=16, error="raw", radius=_lib.TRAY_DENOISE_RADIUS, patch=_lib.TRAY_DENOISE_PATCH,
                            k=_lib.TRAY_DENOISE_K, max_ratio=None):
        """config.select_blocks of the frame rendered to a noise threshold (tray_render_noise_target_device): every tile takes the
        power-of-two prefix [0, n_t) of the round_spp(config.spp)-sample LowDiscrepancy frame, min_spp <= n_t <= that spp, at which its
        two-buffer error drops below `threshold`. error="filtered" takes that error from the two cross-filtered halves of the films instead
        (tray_render_noise_target_filtered_device with radius, patch, k): the rule for a frame that will be denoised. The image (even + odd film,
        unfiltered either way) is added into rt. max_ratio (a power of two >= 2) bounds the ratio of n_t between neighbouring tiles
        (tray_scene_set_noise_ratio, for this call alone), so that no border pixel's weight is cancelled by a neighbour's negative filter lobes.
        Returns (tile_samples, tile_error): numpy arrays of n_t and the last error per tile, in BlockQueue order. LowDiscrepancy only (TrayError
        TRAY_E_UNSUPPORTED otherwise)."""
        import torch
        if error not in ("raw", "filtered"):
            raise ValueError(f"error must be 'raw' or 'filtered', not {error!r}")
        dev = scene.device_scene(config.current_frame, self.device)
        spp = self._select_sampler(dev, config.spp)
        start, count = (int(v) for v in config.select_blocks)
        w, h = rt.dimensions()
        n = len(BlockQueue((w, h), (8, 8), (start, count)).blocks)
        with torch.cuda.device(self.device):
            even = torch.zeros((h, w, 4), dtype=torch.float32, device=f"cuda:{self.device}")
            odd = torch.zeros_like(even)
            samples, err, _ = self._noise_target_device(dev, start, count, min_spp, spp, threshold, even, odd, n, error, radius, patch, k, False, max_ratio)
            rt.add_pixels((even + odd).reshape(-1).cpu().numpy())
        t = self._keep_timing(dev)
        if t is not None:
            print(f"Frame {config.current_frame}: rendering took {t.render_ms * 1e-3:.4f}s")
        return samples, err

    def _filter_call(self, stem, film, middle, outs, scratch_stem=None, scratch_args=()):
        """The one device call of every filter: tray_denoise_<stem>_device(w, h, *middle, *outs, scratch, stream) on the current stream (stem "":
        tray_denoise_device), the scratch buffer sized by the call's own tray_denoise_<stem>_scratch_bytes(w, h, *scratch_args), or by
        scratch_stem's. film: one (h, w, 4) float32 tensor of the call, for the size and the device; middle: the arguments between the size and
        the outputs as the C call takes them; outs: the output tensors, or how many to make, like `film`. Returns the tuple of outputs."""
        import torch
        h, w = int(film.shape[0]), int(film.shape[1])
        name = lambda stem_, last: "_".join(part for part in ("tray_denoise", stem_, last) if part)
        with torch.cuda.device(self.device):
            if isinstance(outs, int):
                outs = tuple(torch.empty_like(film) for _ in range(outs))
            nbytes = getattr(lib(), name(stem if scratch_stem is None else scratch_stem, "scratch_bytes"))(w, h, *scratch_args)
            scratch, stream = _scratch(nbytes, film.device), _current_stream()
            check(lib().tray_init(self.device))   # (the filter runs on the library's current device)
            check(getattr(lib(), name(stem, "device"))(w, h, *middle, *[_ptr(t) for t in outs], _ptr(scratch), stream))
            torch.cuda.current_stream().synchronize()   # (scratch goes out of scope here)
        return outs

    def _denoise_device(self, even, odd, radius, patch, k, second=None, albedo=None):
        """tray_denoise_device of two (h, w, 4) float32 tensors of this device on the current stream, or, with second = (radius2, patch2, k2),
        tray_denoise_two_pass_device; with an albedo film (a third such tensor) tray_denoise_demodulated_device of either; returns the output
        tensor"""
        r2, f2, k2 = (0, 0, 1.0) if second is None else second   # (radius2 == 0: one pass)
        films, first, again = (_ptr(even), _ptr(odd)), (int(radius), int(patch), float(k)), (int(r2), int(f2), float(k2))
        if albedo is not None:
            return self._filter_call("demodulated", even, (*films, _ptr(albedo), *first, *again), 1, scratch_args=again[:1])[0]
        return self._filter_call("" if second is None else "two_pass", even, (*films, *first, *(() if second is None else again)), 1)[0]

    @staticmethod
    def _second_pass(what, passes, radius2, patch2, k2):
        """None for one pass, (radius2, patch2, k2) for two"""
        if passes not in (1, 2):
            raise ValueError(f"{what}: passes must be 1 or 2, not {passes!r}")
        return None if passes == 1 else (radius2, patch2, k2)

    def _films_on_device(self, what, frames, centre=0, albedos=None, guides=None, words=_FRAMES):
        """The intake of every filter call: `frames` is a list of (even, odd) pairs of (h, w, 4) films, `albedos` one film per frame, `guides` one
        (guide_a, guide_b) pair per frame -- numpy arrays, uploaded once, or torch tensors of this device, taken as they are --, all of one kind and
        one size. Returns (as_numpy, rows): per frame the tuple (even, odd[, albedo][, guide_a, guide_b]) of contiguous float32 tensors, frames[centre]
        first. A pair whose two films share their storage gets a copy of its second. `what` and `words` (_FRAMES for lists of frames, _FILMS for one
        frame's films) are the caller's name and nouns in the refusals."""
        import torch
        dev = f"cuda:{self.device}"
        is_numpy = lambda x: isinstance(x, np.ndarray)

        def on_device(x):
            if is_numpy(x):
                return torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(dev)
            if x.device != torch.device(dev):
                raise ValueError(f"{what}: the films must live on {dev}")
            return x.to(torch.float32).contiguous()

        def pairs(listed):
            out = []
            for even, odd in listed:
                if is_numpy(even) != is_numpy(odd):
                    raise TypeError(f"{what}: even and odd must both be numpy arrays or both be torch tensors")
                e, o = on_device(even), on_device(odd)
                if o.data_ptr() == e.data_ptr():
                    o = o.clone()
                if e.dim() != 3 or e.shape[2] != 4 or e.shape != o.shape:
                    raise ValueError(f"{what}: even and odd must be two (h, w, 4) films of one size")
                out.append((e, o))
            if len({is_numpy(even) for even, _ in listed}) != 1:
                raise TypeError(f"{what}: the frames must all be numpy arrays or all be torch tensors")
            if any(e.shape != out[0][0].shape for e, _ in out):
                raise ValueError(f"{what}: the frames must be of one size")
            return out

        frames, c = list(frames), int(centre)
        albedos, guides = (None if x is None else list(x) for x in (albedos, guides))
        if guides is not None and len(guides) != len(frames):
            raise ValueError(f"{what}: guides must hold one pair of films per frame")
        if not 0 <= c < len(frames):
            raise ValueError(f"{what}: centre must index frames")
        rows = pairs(frames)
        as_numpy, size = is_numpy(frames[0][0]), rows[0][0].shape
        if albedos is not None:
            if len(albedos) != len(frames):
                raise ValueError(f"{what}: albedos must hold one albedo film per frame")
            kinds = TypeError(f"{what}: the {words['frames']} and the {words['albedo']} must all be numpy arrays or all be torch tensors")
            mixed = any(is_numpy(a) != as_numpy for a in albedos)
            if mixed and words["albedo_kind_first"]:
                raise kinds
            alb = []
            for a in albedos:
                alb.append(on_device(a))
                if alb[-1].dim() != 3 or alb[-1].shape[2] != 4:
                    raise ValueError(f"{what}: {words['film']}")
            if mixed:
                raise kinds
            if any(a.shape != size for a in alb):
                raise ValueError(f"{what}: the {words['albedo']} must have the {words['frames']}' size")
            rows = [row + (a,) for row, a in zip(rows, alb)]
        if guides is not None:
            gpairs = pairs(guides)
            if is_numpy(guides[0][0]) != as_numpy:
                raise TypeError(f"{what}: the {words['frames']} and the {words['guides']} must all be numpy arrays or all be torch tensors")
            if gpairs[0][0].shape != size:
                raise ValueError(f"{what}: the {words['guides']} must have the {words['frames']}' size")
            rows = [row + g for row, g in zip(rows, gpairs)]
        return as_numpy, [rows[c]] + rows[:c] + rows[c + 1:]

    def denoise(self, even, odd, radius=_lib.TRAY_DENOISE_RADIUS, patch=_lib.TRAY_DENOISE_PATCH, k=_lib.TRAY_DENOISE_K, passes=1,
                radius2=_lib.TRAY_DENOISE_RADIUS2, patch2=_lib.TRAY_DENOISE_PATCH2, k2=_lib.TRAY_DENOISE_K2, albedo=None):
        """The dual-buffer NL-means filter of include/trayhip.h (tray_denoise_device) of two half films, e.g. the even and odd film of a
        noise-target render: two (h, w, 4) float32 RGBW arrays -- numpy arrays or torch tensors on this device -- in, the same kind out: an RGBW
        film of weight 1. Pixels of weight <= 0 or with a non-finite component count as missing and are filled from their neighbourhood.
        passes=2 (tray_denoise_two_pass_device): a second pass of (radius2, patch2, k2) takes its weights from the first pass's output and
        averages the films again. albedo: a first-hit albedo film of the same frame (render_first_hit), of the films' kind and size: the
        colour is divided by it, the remainder filtered and the texture multiplied back in (tray_denoise_demodulated_device)."""
        second = self._second_pass("denoise", passes, radius2, patch2, k2)
        as_numpy, ((e, o, *alb),) = self._films_on_device("denoise", [(even, odd)], albedos=None if albedo is None else [albedo], words=_FILMS)
        return _as_given(as_numpy, self._denoise_device(e, o, radius, patch, k, second, *alb))

    def denoise_guided(self, even, odd, guide_a, guide_b, radius=_lib.TRAY_DENOISE_RADIUS2, patch=_lib.TRAY_DENOISE_PATCH2, k=_lib.TRAY_DENOISE_K2):
        """denoise() with the weights measured on another pair of films (tray_denoise_guided_device): the patch distances come from (guide_a,
        guide_b), e.g. denoise_halves() of the same films, the averaged colours from (even, odd). Films in and out as for denoise(), all four of
        one kind and one size. With the films as their own guide the image is denoise()'s to the bit."""
        as_numpy, (films,) = self._films_on_device("denoise_guided", [(even, odd)], guides=[(guide_a, guide_b)], words=_FILMS)
        out, = self._filter_call("guided", films[0], (*[_ptr(t) for t in films], int(radius), int(patch), float(k)), 1)
        return _as_given(as_numpy, out)

    def _denoise_halves_device(self, e, o, radius, patch, k, fa, fb):
        """tray_denoise_halves_device over every block of two tensors of this device on the current stream, into the tensors fa and fb"""
        self._filter_call("halves", e, (_ptr(e), _ptr(o), int(radius), int(patch), float(k), None, 0), (fa, fb), scratch_stem="")

    def denoise_halves(self, even, odd, radius=_lib.TRAY_DENOISE_RADIUS, patch=_lib.TRAY_DENOISE_PATCH, k=_lib.TRAY_DENOISE_K):
        """The two cross-filtered halves (A, B) of denoise()'s filter (tray_denoise_halves_device), films in and out as there: (A.rgb + B.rgb) / 2
        is denoise()'s image to the bit, a half's weight is 1 where it exists and 0 where no neighbour had weight, and |A - B| / 2 is a per-pixel
        confidence map of the denoised frame."""
        import torch
        as_numpy, ((e, o),) = self._films_on_device("denoise_halves", [(even, odd)], words=_FILMS)
        fa, fb = torch.empty_like(e), torch.empty_like(e)
        self._denoise_halves_device(e, o, radius, patch, k, fa, fb)
        return _as_given(as_numpy, (fa, fb))

    def render_denoised(self, scene, rt, config, threshold=None, min_spp=16, radius=_lib.TRAY_DENOISE_RADIUS, patch=_lib.TRAY_DENOISE_PATCH,
                        k=_lib.TRAY_DENOISE_K, error="raw", passes=1, radius2=_lib.TRAY_DENOISE_RADIUS2, patch2=_lib.TRAY_DENOISE_PATCH2,
                        k2=_lib.TRAY_DENOISE_K2, demodulate=False, feature_spp=None, max_ratio=None):
        """config.select_blocks of the frame rendered as two half films and denoised on the device (tray_denoise_device); the RGBW output (weight 1)
        is added into rt. With `threshold` the films are the even / odd film of a noise-target render (see render_noise_target; error="filtered"
        stops on the error of the denoised image and takes the output from that same call) and (tile_samples, tile_error) is returned; without it
        they are the sample ranges [0, spp / 2) and [spp / 2, spp) of the round_spp(config.spp)-sample frame (spp >= 2) and None is returned.
        passes=2 filters the films as denoise(passes=2) does; the stopping rule of error="filtered" measures one pass's image, so the two do not
        combine. demodulate=True divides the colour by the frame's first-hit albedo before the filter and multiplies it back in afterwards
        (denoise(albedo=...)): the albedo film is rendered from the samples [0, feature_spp or spp) of the same frame and seed; it does not
        combine with error="filtered" either. max_ratio bounds the ratio of n_t between neighbouring tiles of the noise-target render (see
        render_noise_target) and needs a threshold. LowDiscrepancy only (TrayError TRAY_E_UNSUPPORTED otherwise)."""
        import torch
        if error not in ("raw", "filtered"):
            raise ValueError(f"error must be 'raw' or 'filtered', not {error!r}")
        if max_ratio is not None and threshold is None:
            raise ValueError("render_denoised: max_ratio bounds a noise-target render and needs a threshold")
        second = self._second_pass("render_denoised", passes, radius2, patch2, k2)
        if second is not None and error == "filtered":
            raise ValueError("render_denoised: error='filtered' stops on one pass's image and takes it from that call; use passes=1 with it")
        if demodulate and error == "filtered":
            raise ValueError("render_denoised: error='filtered' stops on the undemodulated image and takes it from that call; use demodulate=False with it")
        if error == "filtered" and threshold is None:
            raise ValueError("render_denoised: error='filtered' is a stopping rule and needs a threshold")
        dev = scene.device_scene(config.current_frame, self.device)
        spp = self._select_sampler(dev, config.spp)
        n_feat = spp if feature_spp is None else int(feature_spp)
        if demodulate and not 1 <= n_feat <= spp:
            raise ValueError(f"render_denoised: feature_spp must lie in [1, {spp}]")
        start, count = (int(v) for v in config.select_blocks)
        w, h = rt.dimensions()
        result, out = None, None
        with torch.cuda.device(self.device):
            even = torch.zeros((h, w, 4), dtype=torch.float32, device=f"cuda:{self.device}")
            odd = torch.zeros_like(even)
            stream = torch.cuda.current_stream().cuda_stream
            if threshold is None:
                if spp < 2:
                    raise ValueError("render_denoised: two half films need spp >= 2")
                for film, rng in ((even, (0, spp // 2)), (odd, (spp // 2, spp))):
                    self.render_samples_device(scene, config.current_frame, (start, count), spp, rng, film.data_ptr(), stream or None)
            else:
                n = len(BlockQueue((w, h), (8, 8), (start, count)).blocks)
                samples, err, out = self._noise_target_device(dev, start, count, min_spp, spp, threshold, even, odd, n, error, radius, patch, k, True, max_ratio)
                result = (samples, err)
            self._keep_timing(dev)   # (the last render call's: the whole noise-target call, or the second range)
            if out is None:
                albedo = None
                if demodulate:
                    albedo, normal, depth = (torch.zeros_like(even) for _ in range(3))
                    self.render_first_hit_device(scene, config.current_frame, (start, count), spp, (0, n_feat), albedo.data_ptr(), normal.data_ptr(),
                                                 depth.data_ptr(), stream or None)
                out = self._denoise_device(even, odd, radius, patch, k, second, *(() if albedo is None else (albedo,)))
            rt.add_pixels(out.reshape(-1).cpu().numpy())
        return result

    def _temporal_call(self, stem, centre, neighbours, first, second=None, halves=False, into=None):
        """tray_denoise_<stem>_device on the current stream, for every temporal call: `centre` and each of `neighbours` (a list, in order) are
        tuples of (h, w, 4) float32 tensors of this device -- (even, odd), then the albedo and / or the (guide_a, guide_b) the call takes --;
        first and the optional second are (radius, radius_t, patch, k). Returns the output tensor, or with `halves` the pair (fa, fb), written
        into `into` if given."""
        n = len(neighbours)
        # host arrays of device pointers, one per film of a frame (never of length 0)
        arrays = [(C.c_void_p * max(n, 1))(*[fr[i].data_ptr() for fr in neighbours]) for i in range(len(centre))]
        params = [v for r, rt, f, k in ([first] if second is None else [first, second]) for v in (int(r), int(rt), int(f), float(k))]
        outs = self._filter_call(stem, centre[0], (*[_ptr(t) for t in centre], n, *arrays, *params), 1 if not halves else 2 if into is None else tuple(into))
        return outs if halves else outs[0]

    def _denoise_temporal_device(self, centre, neighbours, radius, radius_t, patch, k, albedos=None):
        """tray_denoise_temporal_device of (even, odd) pairs; albedos: the albedo tensors of the centre and of the neighbours, in that order
        (tray_denoise_temporal_demodulated_device)"""
        if albedos is None:
            return self._temporal_call("temporal", centre, neighbours, (radius, radius_t, patch, k))
        triples = [tuple(pair) + (a,) for pair, a in zip([centre] + list(neighbours), albedos)]
        return self._temporal_call("temporal_demodulated", triples[0], triples[1:], (radius, radius_t, patch, k))

    def _denoise_temporal_halves_device(self, centre, neighbours, radius, radius_t, patch, k, into=None):
        """tray_denoise_temporal_halves_device of (even, odd) pairs; returns (fa, fb), written into `into` if given"""
        return self._temporal_call("temporal_halves", centre, neighbours, (radius, radius_t, patch, k), halves=True, into=into)

    def _denoise_temporal_demodulated_halves_device(self, centre, neighbours, radius, radius_t, patch, k, into=None):
        """tray_denoise_temporal_demodulated_halves_device of (even, odd, albedo) triples; returns (fa, fb), written into `into` if given"""
        return self._temporal_call("temporal_demodulated_halves", centre, neighbours, (radius, radius_t, patch, k), halves=True, into=into)

    def denoise_temporal_demodulated_halves(self, frames, albedos, centre, radius=_lib.TRAY_DENOISE_RADIUS, radius_t=_lib.TRAY_DENOISE_RADIUS_T,
                                            patch=_lib.TRAY_DENOISE_PATCH, k=_lib.TRAY_DENOISE_K):
        """denoise_temporal_halves() of the frames divided by their own albedo films (tray_denoise_temporal_demodulated_halves_device): frames and
        albedos in as for denoise_temporal_demodulated(), two films out. The halves are NOT multiplied by the centre's texture: they are the
        guides of denoise_temporal_demodulated_guided(). A one-element list gives a frame's own halves in that domain."""
        as_numpy, triples = self._films_on_device("denoise_temporal_demodulated_halves", frames, centre, albedos)
        return _as_given(as_numpy, self._denoise_temporal_demodulated_halves_device(triples[0], triples[1:], radius, radius_t, patch, k))

    def denoise_temporal_demodulated_guided(self, frames, albedos, guides, centre, radius=_lib.TRAY_DENOISE_RADIUS2, radius_t=_lib.TRAY_DENOISE_RADIUS_T2,
                                            patch=_lib.TRAY_DENOISE_PATCH2, k=_lib.TRAY_DENOISE_K2):
        """denoise_temporal_guided() of the frames divided by their own albedo films, times frames[centre]'s texture
        (tray_denoise_temporal_demodulated_guided_device): `guides` holds one (guide_a, guide_b) pair per frame, already in the demodulated domain,
        e.g. denoise_temporal_demodulated_halves() of the centre and of every other frame alone. All films of one kind and size, all different."""
        as_numpy, rows = self._films_on_device("denoise_temporal_demodulated_guided", frames, centre, albedos, guides)
        return _as_given(as_numpy, self._temporal_call("temporal_demodulated_guided", rows[0], rows[1:], (radius, radius_t, patch, k)))

    def _denoise_temporal(self, what, frames, centre, albedos, first, second):
        """denoise_temporal and denoise_temporal_demodulated after their own refusals: the films taken in, and the one call that `albedos` (a list,
        or None) and `second` ((radius2, radius_t2, patch2, k2), or None) select"""
        as_numpy, rows = self._films_on_device(what, frames, centre, albedos)
        stem = "temporal" + ("_demodulated" if albedos is not None else "") + ("_two_pass" if second is not None else "")
        return _as_given(as_numpy, self._temporal_call(stem, rows[0], rows[1:], first, second))

    def denoise_temporal_demodulated(self, frames, albedos, centre, radius=_lib.TRAY_DENOISE_RADIUS, radius_t=_lib.TRAY_DENOISE_RADIUS_T,
                                     patch=_lib.TRAY_DENOISE_PATCH, k=_lib.TRAY_DENOISE_K, passes=2, radius2=_lib.TRAY_DENOISE_RADIUS2,
                                     radius_t2=_lib.TRAY_DENOISE_RADIUS_T2, patch2=_lib.TRAY_DENOISE_PATCH2, k2=_lib.TRAY_DENOISE_K2):
        """denoise_temporal() on albedo-demodulated films with a second pass over all frames, for a textured, moving sequence: `frames` and `albedos`
        as denoise_temporal(albedos=...) takes them, numpy arrays or tensors of this device, the same kind out. Every frame's colour is divided by
        its own albedo, the remainders are filtered as denoise_temporal(passes=2) filters films, and frames[centre]'s texture is multiplied back
        in (tray_denoise_temporal_demodulated_two_pass_device). passes=1 is denoise_temporal(albedos=...), to the bit
        (tray_denoise_temporal_demodulated_device). A one-element list gives denoise(albedo=..., passes=2)'s image to the bit."""
        second = self._second_pass("denoise_temporal_demodulated", passes, radius2, patch2, k2)
        return self._denoise_temporal("denoise_temporal_demodulated", frames, centre, list(albedos), (radius, radius_t, patch, k),
                                      second and (radius2, radius_t2, patch2, k2))

    def denoise_temporal_halves(self, frames, centre, radius=_lib.TRAY_DENOISE_RADIUS, radius_t=_lib.TRAY_DENOISE_RADIUS_T, patch=_lib.TRAY_DENOISE_PATCH,
                                k=_lib.TRAY_DENOISE_K):
        """The two cross-filtered halves (A, B) of denoise_temporal()'s filter (tray_denoise_temporal_halves_device), frames in as there and two
        films out as from denoise_halves(): (A.rgb + B.rgb) / 2 is denoise_temporal()'s image to the bit, and a one-element list gives
        denoise_halves()'s films to the bit."""
        as_numpy, pairs = self._films_on_device("denoise_temporal_halves", frames, centre)
        return _as_given(as_numpy, self._denoise_temporal_halves_device(pairs[0], pairs[1:], radius, radius_t, patch, k))

    def denoise_temporal_guided(self, frames, guides, centre, radius=_lib.TRAY_DENOISE_RADIUS2, radius_t=_lib.TRAY_DENOISE_RADIUS_T2,
                                patch=_lib.TRAY_DENOISE_PATCH2, k=_lib.TRAY_DENOISE_K2):
        """denoise_temporal() with the weights measured on guides (tray_denoise_temporal_guided_device): `guides` holds one (guide_a, guide_b) pair
        per frame, e.g. denoise_temporal_halves() of the centre and denoise_halves() of every other frame; the patch distances come from them, the
        averaged colours from `frames`. All films of one kind and size. With the frames as their own guides the image is denoise_temporal()'s to
        the bit; a one-element list gives denoise_guided()'s."""
        as_numpy, rows = self._films_on_device("denoise_temporal_guided", frames, centre, guides=guides)
        return _as_given(as_numpy, self._temporal_call("temporal_guided", rows[0], rows[1:], (radius, radius_t, patch, k)))

    def denoise_temporal(self, frames, centre, radius=_lib.TRAY_DENOISE_RADIUS, radius_t=_lib.TRAY_DENOISE_RADIUS_T, patch=_lib.TRAY_DENOISE_PATCH,
                         k=_lib.TRAY_DENOISE_K, albedos=None, passes=1, radius2=_lib.TRAY_DENOISE_RADIUS2, radius_t2=_lib.TRAY_DENOISE_RADIUS_T2,
                         patch2=_lib.TRAY_DENOISE_PATCH2, k2=_lib.TRAY_DENOISE_K2):
        """denoise() for a frame of a sequence (tray_denoise_temporal_device): `frames` is a list of (even, odd) half-film pairs of consecutive frames,
        as denoise() takes them; frames[centre] is filtered, and its filter also searches a window of radius_t in each of the other frames, in
        list order (at most 8 of them). Returns the same kind it was given. A one-element list gives denoise()'s image to the bit.
        albedos: a list of first-hit albedo films (render_first_hit), one per frame, of the frames' kind and size: every frame's colour is divided
        by its own albedo, the remainders are filtered together and frames[centre]'s texture is multiplied back in
        (tray_denoise_temporal_demodulated_device); a one-element list then gives denoise(albedo=...)'s image to the bit.
        passes=2 (tray_denoise_temporal_two_pass_device): a second pass of (radius2, radius_t2, patch2, k2) over all frames takes its weights from
        first-pass output -- frames[centre]'s from denoise_temporal_halves(), every other frame's from its own denoise_halves() -- and averages
        the films again; a one-element list then gives denoise(passes=2)'s image to the bit. It does not combine with albedos."""
        second = self._second_pass("denoise_temporal", passes, radius2, patch2, k2)
        if second is not None and albedos is not None:
            raise ValueError("denoise_temporal: passes=2 filters the films as they are; use albedos=None with it")
        return self._denoise_temporal("denoise_temporal", frames, centre, albedos, (radius, radius_t, patch, k), second and (radius2, radius_t2, patch2, k2))

    def _render_sequence(self, what, scene, config, frames, reach, first, second, albedo, feature_spp):
        """The loop of both sequence generators, with its checks in `what`'s name. Every frame of `frames` is rendered once into films of its own: its
        two half films; with `albedo` its first-hit albedo film, from the samples [0, feature_spp or spp); with a second pass two more for its own
        first-pass halves, computed right after the renders. They are held while a later frame's window reaches them and rendered into again
        afterwards. Every frame is then filtered with the other frames of its window in ascending order: by one call with first = (radius, radius_t,
        patch, k), or, with second = (radius2, radius_t2, patch2, k2), by its halves over the window (into the one pilot pair) and the guided call.
        Yields (frame, rgbw)."""
        import torch
        frames, reach = [int(f) for f in frames], int(reach)
        if any(b != a + 1 for a, b in zip(frames, frames[1:])):
            raise ValueError(f"{what}: frames must be consecutive frame numbers")
        if not 0 <= 2 * reach <= _lib.TRAY_DENOISE_MAX_NEIGHBOURS:
            raise ValueError(f"{what}: 0 <= reach <= {_lib.TRAY_DENOISE_MAX_NEIGHBOURS // 2}")
        if not frames:
            return
        spp = self._select_sampler(scene.device_scene(frames[0], self.device), config.spp)
        if spp < 2:
            raise ValueError(f"{what}: two half films need spp >= 2")
        n_feat = spp if feature_spp is None else int(feature_spp)
        if albedo and not 1 <= n_feat <= spp:
            raise ValueError(f"{what}: feature_spp must lie in [1, {spp}]")
        film = scene.flatten(frames[0]).contents.film
        w, h = int(film.width), int(film.height)
        n = 3 if albedo else 2   # the films of a frame that a filter reads: (even, odd[, albedo]); its own halves (fa, fb) follow them
        held, spare = {}, []   # frame -> its films on the device; the films of frames that are done, to be rendered into again
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream().cuda_stream
            new_film = lambda: torch.empty((h, w, 4), dtype=torch.float32, device=f"cuda:{self.device}")
            throw_away = (new_film(), new_film()) if albedo else None   # the normal and depth films nobody reads
            pilot = (new_film(), new_film()) if second is not None else None   # the halves of the frame in hand over all its frames
            for f in frames:
                window = range(max(frames[0], f - reach), min(frames[-1], f + reach) + 1)
                for g in window:
                    if g not in held:
                        films = spare.pop() if spare else tuple(new_film() for _ in range(n if second is None else n + 2))
                        for half, rng in zip(films, ((0, spp // 2), (spp // 2, spp))):
                            half.zero_()
                            self.render_samples_device(scene, g, config.select_blocks, spp, rng, half.data_ptr(), stream or None)
                        if albedo:
                            for t in (films[2],) + throw_away:
                                t.zero_()
                            self.render_first_hit_device(scene, g, config.select_blocks, spp, (0, n_feat), films[2].data_ptr(),
                                                         throw_away[0].data_ptr(), throw_away[1].data_ptr(), stream or None)
                        # the frame's own first-pass halves, once: the guide it brings to its neighbours' second passes
                        if second is not None and albedo:
                            self._denoise_temporal_demodulated_halves_device(films[:3], [], *first, films[3:])
                        elif second is not None:
                            self._denoise_halves_device(films[0], films[1], first[0], first[2], first[3], films[2], films[3])
                        held[g] = films
                mine, others = held[f], [held[g] for g in window if g != f]
                if second is None:
                    out = self._denoise_temporal_device(mine[:2], [fr[:2] for fr in others], *first, *(([fr[2] for fr in [mine] + others],) if albedo else ()))
                else:
                    halves = self._denoise_temporal_demodulated_halves_device if albedo else self._denoise_temporal_halves_device
                    halves(mine[:n], [fr[:n] for fr in others], *first, pilot)
                    out = self._temporal_call("temporal_demodulated_guided" if albedo else "temporal_guided", mine[:n] + pilot, others, second)
                for g in [g for g in held if g <= f - reach]:   # (no later frame's window reaches back to them)
                    spare.append(held.pop(g))
                yield f, out.cpu().numpy()

    def render_sequence_denoised(self, scene, config, frames, reach=1, radius=_lib.TRAY_DENOISE_RADIUS, radius_t=_lib.TRAY_DENOISE_RADIUS_T,
                                 patch=_lib.TRAY_DENOISE_PATCH, k=_lib.TRAY_DENOISE_K, demodulate=False, feature_spp=None, passes=1,
                                 radius2=_lib.TRAY_DENOISE_RADIUS2, radius_t2=_lib.TRAY_DENOISE_RADIUS_T2, patch2=_lib.TRAY_DENOISE_PATCH2,
                                 k2=_lib.TRAY_DENOISE_K2):
        """Generator over the consecutive frame numbers `frames`: config.select_blocks of every frame rendered once as its two half films (the sample
        ranges [0, spp / 2) and [spp / 2, spp) of the round_spp(config.spp)-sample frame, as render_denoised without a threshold) and filtered
        with the up to `reach` frames before and after it that belong to `frames` (denoise_temporal, the neighbours in ascending frame order);
        yields (frame, rgbw) with rgbw an (h, w, 4) numpy array of weight 1. At most 2 reach + 1 film pairs live on the device. One seed, self.seed:
        the frame number already keys the sampler. demodulate=True also renders every frame's first-hit albedo film once, from the samples
        [0, feature_spp or spp) of that frame, and filters with denoise_temporal(albedos=...): at most 2 reach + 1 albedo films live on the device
        beside one throw-away normal and depth film. passes=2 filters every frame as denoise_temporal(passes=2) filters the films rendered here,
        to the bit: every frame's own first-pass halves (denoise_halves) are computed once, when it is rendered, and kept with its films (at most
        2 reach + 1 such pairs and one pair for the centre's halves over all frames); it does not combine with demodulate.
        LowDiscrepancy only (TrayError TRAY_E_UNSUPPORTED otherwise)."""
        second = self._second_pass("render_sequence_denoised", passes, radius2, patch2, k2)
        if second is not None and demodulate:
            raise ValueError("render_sequence_denoised: passes=2 filters the films as they are; use demodulate=False with it")
        yield from self._render_sequence("render_sequence_denoised", scene, config, frames, reach, (radius, radius_t, patch, k),
                                         second and (radius2, radius_t2, patch2, k2), demodulate, feature_spp)

    def render_sequence_demodulated(self, scene, config, frames, reach=1, passes=2, feature_spp=None, radius=_lib.TRAY_DENOISE_RADIUS,
                                    radius_t=_lib.TRAY_DENOISE_RADIUS_T, patch=_lib.TRAY_DENOISE_PATCH, k=_lib.TRAY_DENOISE_K,
                                    radius2=_lib.TRAY_DENOISE_RADIUS2, radius_t2=_lib.TRAY_DENOISE_RADIUS_T2, patch2=_lib.TRAY_DENOISE_PATCH2,
                                    k2=_lib.TRAY_DENOISE_K2):
        """render_sequence_denoised() with albedo demodulation AND the second pass over all frames, for a textured, moving sequence: a generator over
        the consecutive frame numbers `frames` that yields (frame, rgbw). Every frame is rendered once -- its two half films as there, its
        first-hit albedo film from the samples [0, feature_spp or spp) --, its own demodulated first-pass halves are computed once, when it is
        rendered (denoise_temporal_demodulated_halves of the frame alone), and every frame is filtered as
        denoise_temporal_demodulated(passes=2) filters the films rendered here, to the bit: the centre's halves over its window's frames, then
        denoise_temporal_demodulated_guided. Films held on the device: at most 5 (2 reach + 1) -- per frame of the window its two half films, its
        albedo film and its two halves, rendered into again when the frame is done --, one throw-away normal and depth film and one pair for the
        centre's halves over all frames: 10 reach + 9. passes=1 is render_sequence_denoised(demodulate=True). LowDiscrepancy only (TrayError
        TRAY_E_UNSUPPORTED otherwise)."""
        second = self._second_pass("render_sequence_demodulated", passes, radius2, patch2, k2)
        if second is None:
            yield from self.render_sequence_denoised(scene, config, frames, reach, radius, radius_t, patch, k, demodulate=True, feature_spp=feature_spp)
            return
        yield from self._render_sequence("render_sequence_demodulated", scene, config, frames, reach, (radius, radius_t, patch, k),
                                         (radius2, radius_t2, patch2, k2), True, feature_spp)

    def render_shard_device(self, scene, frame, shard, n_shards, spp, rgbw_ptr, chunk_tiles=16, stream=None):
        """One rank's share of a frame (round-robin chunks of the Morton queue); merge = sum over ranks."""
        dev = scene.device_scene(frame, self.device)
        spp = self._select_sampler(dev, spp)
        check(lib().tray_render_shard_device(dev, int(shard), int(n_shards), int(chunk_tiles), int(spp), self.seed,
                                             C.c_void_p(int(rgbw_ptr)), C.c_void_p(int(stream)) if stream else None))
        return dev

    def render_multi(self, scene, rt, config, devices, partition="tiles"):
        """One frame on several GPUs of this process: tiles sharded round-robin over `devices` (partition="tiles"), or every tile on every
        device with device d rendering the samples multi.shard_samples(spp, d, len(devices)) gives it (partition="samples": equal work per
        device; LowDiscrepancy only), the per-device films summed onto
        the first one by RCCL inside the library (tray_render_frame_multi; the master's Image::add_blocks merge,
        exec/distrib/master.rs:124-163, film/image.rs:36-50), the result added into rt. Returns (per-device timings, reduce ms).
        The per-device scenes and the communicators are kept between calls: another frame of the same scene on the same devices
        is a tray_multi_update_frame (scene.rs:152-176), not a new ncclCommInitAll. close_multi() releases them."""
        key = tuple(int(d) for d in devices)
        # the cached device copies belong to ONE scene object, held by a strong reference and compared by identity: an id() alone
        # could be reused by another Scene allocated at the same address after this one was collected, and that scene's frame would
        # then be grafted onto the old one's meshes and tables by tray_multi_update_frame
        if self._multi is not None and (self._multi_scene is not scene or self._multi_key != key):
            self.close_multi()
        flat = scene.flatten(config.current_frame)
        if self._multi is None:
            ids = (C.c_int * len(devices))(*[int(d) for d in devices])
            m = C.c_void_p()
            check(lib().tray_multi_create(flat, len(devices), ids, C.byref(m)))
            self._multi, self._multi_key, self._multi_frame, self._multi_scene = m, key, config.current_frame, scene
        elif self._multi_frame != config.current_frame:
            try:
                check(lib().tray_multi_update_frame(self._multi, flat))
            except TrayError:
                self.close_multi()
                raise
            self._multi_frame = config.current_frame
        spp = self._select_sampler(self._multi, config.spp, multi=True)
        if partition not in _PARTITIONS:
            raise ValueError(f"render_multi: partition must be one of {sorted(_PARTITIONS)}")
        check(lib().tray_multi_set_partition(self._multi, _PARTITIONS[partition]))
        check(lib().tray_render_frame_multi(self._multi, spp, self.seed, rt.pixels.ctypes.data))
        per = (_lib.TrayKernelTiming * len(devices))()
        ms = C.c_float()
        check(lib().tray_multi_timing(self._multi, per, C.byref(ms)))
        return list(per), float(ms.value)

    def close_multi(self):
        if self._multi is not None:
            lib().tray_multi_destroy(self._multi)
            self._multi = None
        self._multi_scene = None

    def __del__(self):
        try:
            self.close_multi()
        except Exception:
            pass

    def schedule(self, scene):
        """the schedule the last render call of `scene` on this device ran with (tray_last_schedule): pool slots, views, slices, bytes"""
        info = _lib.TrayScheduleInfo()
        check(lib().tray_last_schedule(scene.device_scene(scene._dev_frame, self.device), C.byref(info)))
        return {name: int(getattr(info, name)) for name, _ in info._fields_}

    def set_wavefront(self, scene, pool_slots=0, views=0, slices=0):
        """tray_scene_set_wavefront on the scene's device copy (0 = the library's own rule)"""
        check(lib().tray_scene_set_wavefront(scene.device_scene(scene._dev_frame, self.device), int(pool_slots), int(views), int(slices)))

    def set_transform_table(self, scene, mode=-1):
        """tray_scene_set_transform_table: 1 = the frame's table of transforms by shutter-time index, 0 = per-path evaluation, -1 = by sample count"""
        check(lib().tray_scene_set_transform_table(scene.device_scene(scene._dev_frame, self.device), int(mode)))

    def timing(self, scene):
        t = _lib.TrayKernelTiming()
        check(lib().tray_last_timing(scene.device_scene(scene._dev_frame, self.device), C.byref(t)))
        self.last_timing = t
        return t
