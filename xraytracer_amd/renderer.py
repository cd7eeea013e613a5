"""Python mirror of HipRenderer (include/xrt/renderer.h) over the C ABI.

``HipRenderer(spp, device).render(scene)`` has the contract of the reference's
``Renderer::render(scene, Uniform, image)`` (Src/renderer.h:15, renderer.cpp:29-99): it
returns the per-pixel mean of ``spp`` samples, seeds ``j + width*i`` per pixel, and drops
NaN / Inf / negative samples.  Everything runs on the GPU through libxrt_hip.so; there is
no CPU fallback.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import abi
from .scenes import SceneBundle


class ProgressiveSession:
    """A frame rendered in passes (xrt_progressive_*): ``add(spp)`` renders spp more samples of every
    pixel, ``frame()`` is the mean of the samples so far — bit for bit what one render() at spp_done
    samples gives.  Made by HipRenderer.progressive(); a context manager.  Uploading a scene or any
    render on the same HipRenderer ends it (add and frame then raise)."""

    def __init__(self, renderer, width, height, variance):
        self._r, self._lib = renderer, renderer._lib
        self.width, self.height, self.variance = width, height, bool(variance)
        self.stats = None   # the last add's xrt_stats: path counters of the session so far, timings of that add

    @property
    def state(self) -> abi.XrtProgressiveState:
        s = abi.XrtProgressiveState()
        self._r._check(self._lib.xrt_progressive_query(self._r.ctx, C.byref(s)), "xrt_progressive_query")
        return s

    @property
    def spp_done(self) -> int:
        return int(self.state.spp_done)

    def add(self, spp: int):
        st = abi.XrtStats()
        self._r._check(self._lib.xrt_progressive_add(self._r.ctx, int(spp), C.byref(st)), "xrt_progressive_add")
        self.stats = self._r.stats = st
        return st

    def frame(self, variance: bool = None):
        """(H, W, 3) float32, and in a session with variance=True also the (H, W) variance plane of
        render_var (which needs spp_done >= 2; variance=False: the frame alone)"""
        want = self.variance if variance is None else bool(variance)
        img = np.zeros((self.height, self.width, 3), np.float32)
        var = np.zeros((self.height, self.width), np.float32) if want else None
        self._r._check(self._lib.xrt_progressive_frame(self._r.ctx, abi.fptr(img), abi.fptr(var) if want else None),
                       "xrt_progressive_frame")
        return (img, var) if want else img

    def frame_device(self, out: int, var: int = None, after_stream=None):
        """the frame into device memory: out H*W*3 float32, var H*W float32 or None (torch tensor
        .data_ptr()); after_stream as for render_var_device"""
        self._r._check(self._lib.xrt_progressive_frame_device(self._r.ctx, C.c_void_p(out or None), C.c_void_p(var or None),
                                                              C.c_void_p(after_stream or None)),
                       "xrt_progressive_frame_device")

    def close(self):
        if self._r is not None and self._r.ctx:
            self._lib.xrt_progressive_end(self._r.ctx)
        self._r = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class HipRenderer:
    def __init__(self, spp: int, device: int = 0, devices=None):
        """device: one GPU; devices: a list of GPUs rendered as one (xrt_create_multi —
        row shards per GPU, frame assembled on devices[0])."""
        self.spp = int(spp)
        self._lib = abi.lib()
        ctx = C.c_void_p()
        if devices is not None:
            devs = (C.c_int * len(devices))(*[int(d) for d in devices])
            rc = self._lib.xrt_create_multi(devs, len(devices), C.byref(ctx))
            what = f"xrt_create_multi(devices={list(devices)})"
        else:
            rc = self._lib.xrt_create(int(device), C.byref(ctx))
            what = f"xrt_create(device={device})"
        if rc != 0:
            raise abi.XrtError(f"{what} failed ({rc}): {self._lib.xrt_last_error(None).decode()}")
        self.ctx = ctx
        self.stats = None
        self._uploaded = None

    def close(self):
        ctx, self.ctx = getattr(self, "ctx", None), None
        if ctx:
            self._lib.xrt_destroy(ctx)

    __del__ = close

    def _check(self, rc, what):
        if rc != 0:
            raise abi.XrtError(f"{what} failed ({rc}): {self._lib.xrt_last_error(self.ctx).decode()}")

    def upload(self, scene: SceneBundle):
        self._check(self._lib.xrt_upload_scene(self.ctx, C.byref(scene.desc)), "xrt_upload_scene")
        cam = scene.camera
        self._check(self._lib.xrt_set_camera(self.ctx, abi.fptr(cam.c2w), C.c_float(cam.scale),
                                             C.c_float(cam.aspect)), "xrt_set_camera")
        dl, ndl = scene.delta_lights()   # always sent: a scene without any clears the context's
        self._check(self._lib.xrt_set_delta_lights(self.ctx, dl, ndl), "xrt_set_delta_lights")
        if scene.medium is not None:
            md = scene.medium.desc()
            if getattr(scene.medium, "sparse", False):
                table, bricks = scene.medium.bricks()
                self._bricks = (table, bricks)   # alive until the library has copied them
                nbz, nby, nbx = table.shape
                bg = abi.XrtBrickGrid(nbx, nby, nbz, table.ctypes.data_as(C.POINTER(C.c_int32)), len(bricks),
                                      abi.fptr(bricks.reshape(-1)))
                self._check(self._lib.xrt_set_medium_bricks(self.ctx, C.byref(md), C.byref(bg)),
                            "xrt_set_medium_bricks")
            else:
                self._check(self._lib.xrt_set_medium(self.ctx, C.byref(md)), "xrt_set_medium")
        self._uploaded = scene

    BVH_INFO = ("bvh_nodes", "bvh_stack", "bvh4_nodes", "bvh4_stack", "two_level", "n_snode", "bvh_tris", "stack_entry")

    def bvh_info(self, scene: SceneBundle) -> dict:
        """What the upload of the scene built for the kernels that walk a hierarchy (xrt_test_bvh_info,
        a self-test that launches nothing): the BVH_INFO values by name."""
        if self._uploaded is not scene:
            self.upload(scene)
        out = (C.c_int32 * 8)()
        self._check(self._lib.xrt_test_bvh_info(self.ctx, out), "xrt_test_bvh_info")
        return dict(zip(self.BVH_INFO, (int(v) for v in out)))

    def params(self, scene, width, height, shard_index=0, shard_count=1, timing=False, integrator=None,
               max_depth=None, schedule="auto", slots_per_wave=0, visits_per_launch=0, group=True,
               accumulate=False, deep="auto", spec=True, whitted_bvh=False, overlap=True, interleave=None,
               fused_var=False, chunks=None):
        """schedule: "auto" (fused k_step when the scene fits in LDS — for small triangle
        scenes with merged shadow + extension traces, for Direct / Normal pixel-parallel
        sample chains (k_pixel) — else the multi-pass wavefront), "step" (the per-slot fused
        schedule also for Direct / Normal), "wavefront" (always k_shade + k_trace) or
        "step_tri" (per-slot fused, one cooperative trace per ray kind instead of the merged
        traces).  slots_per_wave / visits_per_launch /
        group fix the merged schedule's launch geometry (0 / True = the library's choice);
        results never depend on them.  accumulate: add the samples to the output buffer's
        current contents before the divide (XRT_FLAG_ACCUMULATE, Renderer::render's contract).
        deep: the two-level trace's BVH walk, "auto", "single" (one lane per queued ray) or
        "quad" (four); results never depend on it.  spec: speculative sample starts in the merged
        schedule's 16-slot launches (GI with one light, every other object a Lambert; spec=False sets XRT_FLAG_NO_SPEC); results
        never depend on it.  whitted_bvh: WhittedIntegrator may render a triangle scene that does
        not fit LDS through its triangle BVH (XRT_FLAG_WHITTED_BVH, XRT_SCHED_WHITTED_BVH) instead
        of refusing it; a scene that fits LDS renders as without it.  overlap: the merged schedule's
        full-wave step launches run in partition groups on streams of their own (overlap=False sets
        XRT_FLAG_NO_OVERLAP: one launch per round); results never depend on it.  interleave: pixels
        interleaved across the merged schedule's path slots (None: the library's rule, large one-level
        renders; True sets XRT_FLAG_INTERLEAVE, any merged render; False sets XRT_FLAG_NO_INTERLEAVE);
        results never depend on it.  fused_var: a variance render (render_var) keeps the schedule
        render() would take with spec=False and without pixel-parallel chains, instead of the
        wavefront (XRT_FLAG_VAR_FUSED); same frame and plane; no effect on any other call.  chunks: the
        merged schedule's whole-wave phase in block-owned chunks (None: the library's rule, large
        interleaved renders of many samples; True sets XRT_FLAG_CHUNKS, any one-level merged render that
        starts at 64 slots per wave; False sets XRT_FLAG_NO_CHUNKS); results never depend on it."""
        if schedule not in ("auto", "step", "wavefront", "step_tri"):
            raise ValueError(f"unknown schedule {schedule!r}")
        if deep not in ("auto", "single", "quad"):
            raise ValueError(f"unknown deep walk {deep!r}")
        p = abi.XrtRenderParams()
        p.integrator = abi.INTEGRATORS[integrator or scene.integrator]
        p.max_depth = scene.max_depth if max_depth is None else max_depth
        p.width, p.height, p.spp = width, height, self.spp
        p.shard_index, p.shard_count = shard_index, shard_count
        p.flags = ((abi.XRT_FLAG_TIMING if timing else 0) | (abi.XRT_FLAG_WAVEFRONT if schedule == "wavefront" else 0) |
                   (abi.XRT_FLAG_NO_MERGED if schedule == "step_tri" else 0) | (0 if group else abi.XRT_FLAG_NO_GROUP) |
                   (abi.XRT_FLAG_NO_PIXEL if schedule in ("step", "step_tri") else 0) |
                   (abi.XRT_FLAG_ACCUMULATE if accumulate else 0) | (0 if spec else abi.XRT_FLAG_NO_SPEC) |
                   (abi.XRT_FLAG_WHITTED_BVH if whitted_bvh else 0) | (0 if overlap else abi.XRT_FLAG_NO_OVERLAP) |
                   (0 if interleave is None else abi.XRT_FLAG_INTERLEAVE if interleave else abi.XRT_FLAG_NO_INTERLEAVE) |
                   (abi.XRT_FLAG_VAR_FUSED if fused_var else 0) |
                   (0 if chunks is None else abi.XRT_FLAG_CHUNKS if chunks else abi.XRT_FLAG_NO_CHUNKS) |
                   {"auto": 0, "single": abi.XRT_FLAG_DEEP_SINGLE, "quad": abi.XRT_FLAG_DEEP_QUAD}[deep])
        p.slots_per_wave, p.visits_per_launch = slots_per_wave, visits_per_launch
        return p

    def render(self, scene: SceneBundle, width: int, height: int, initial=None, **kw) -> np.ndarray:
        """Render into a host (H, W, 3) float32 image.  initial: the Image's prior contents,
        accumulated into in place as Renderer::render does (XRT_FLAG_ACCUMULATE)."""
        if self._uploaded is not scene:
            self.upload(scene)
        p = self.params(scene, width, height, accumulate=initial is not None, **kw)
        img = np.zeros((height, width, 3), np.float32)
        if initial is not None:
            img[...] = initial
        st = abi.XrtStats()
        self._check(self._lib.xrt_render(self.ctx, C.byref(p), abi.fptr(img), C.byref(st)), "xrt_render")
        self.stats = st
        return img

    def progressive(self, scene: SceneBundle, width: int, height: int, variance: bool = False, **kw) -> ProgressiveSession:
        """Open a progressive session (xrt_progressive_begin) and return it: add(spp), frame(),
        frame_device(), spp_done, state, stats, close().  variance: also sum the luminance moments, so
        frame() returns (img, var) as render_var does.  self.spp is ignored.  The schedule is render()'s
        with spec=False and without pixel-parallel chains; WhittedIntegrator, accumulate and a
        multi-device renderer are refused.  kw: params()'s."""
        if self._uploaded is not scene:
            self.upload(scene)
        p = self.params(scene, width, height, **kw)
        self._check(self._lib.xrt_progressive_begin(self.ctx, C.byref(p), abi.XRT_PROGRESSIVE_VARIANCE if variance else 0),
                    "xrt_progressive_begin")
        return ProgressiveSession(self, width, height, variance)

    def render_var(self, scene: SceneBundle, width: int, height: int, **kw):
        """The frame and the variance of each pixel's mean luminance (xrt_render_var): ((H, W, 3),
        (H, W)) float32.  The frame is render()'s, bit for bit; the variance plane is what
        denoise_var takes as `variance`.  self.spp must be at least 2.  The path integrators run
        the wavefront schedule whatever the schedule keywords say, unless fused_var=True: then
        they run the fused or merged schedule render() would choose with spec=False and
        schedule="step" (or "step_tri") and the other schedule keywords count; the frame and the
        plane are the same bits either way.  accumulate is refused.  kw: params()'s."""
        if self._uploaded is not scene:
            self.upload(scene)
        p = self.params(scene, width, height, **kw)
        img = np.zeros((height, width, 3), np.float32)
        var = np.zeros((height, width), np.float32)
        st = abi.XrtStats()
        self._check(self._lib.xrt_render_var(self.ctx, C.byref(p), abi.fptr(img), abi.fptr(var), C.byref(st)),
                    "xrt_render_var")
        self.stats = st
        return img, var

    def render_var_device(self, scene: SceneBundle, width: int, height: int, out_ptr: int, var_ptr: int,
                          after_stream=None, **kw):
        """render_var into device buffers (xrt_render_var_device): out_ptr H*W*3 float32, var_ptr
        H*W float32 (torch tensor .data_ptr()).  after_stream as for render_aov_device.  fused_var
        as for render_var.  Returns the stats when both planes are complete."""
        if self._uploaded is not scene:
            self.upload(scene)
        p = self.params(scene, width, height, **kw)
        st = abi.XrtStats()
        self._check(self._lib.xrt_render_var_device(self.ctx, C.byref(p), C.c_void_p(out_ptr or None),
                                                    C.c_void_p(var_ptr or None), C.c_void_p(after_stream or None),
                                                    C.byref(st)), "xrt_render_var_device")
        self.stats = st
        return st

    _AOV_SHAPES = {"albedo": (3,), "normal": (3,), "depth": (), "alpha": (), "object": ()}

    def render_aov(self, scene: SceneBundle, width: int, height: int,
                   planes=("albedo", "normal", "depth", "alpha", "object"), **kw) -> dict:
        """First-hit guide buffers (xrt_render_aov) through the render's own jittered camera
        rays at self.spp: a dict of the requested planes — albedo, normal (H, W, 3), depth,
        alpha (H, W) float32 sample means, object (H, W) int32 (sample 0's object, -1 = miss).
        Mean depth over the hits is depth / alpha.  kw: shard_index, shard_count, timing; the
        integrator and the schedule keywords have no effect."""
        planes = tuple(planes)
        bad = [n for n in planes if n not in self._AOV_SHAPES]
        if bad:
            raise ValueError(f"unknown guide planes {bad}")
        if self._uploaded is not scene:
            self.upload(scene)
        p = self.params(scene, width, height, **kw)
        out = {n: np.zeros((height, width) + self._AOV_SHAPES[n], np.int32 if n == "object" else np.float32)
               for n in planes}
        bufs = abi.XrtAovBuffers(**{n: a.ctypes.data for n, a in out.items()})
        st = abi.XrtStats()
        self._check(self._lib.xrt_render_aov(self.ctx, C.byref(p), C.byref(bufs), C.byref(st)), "xrt_render_aov")
        self.stats = st
        return out

    def render_aov_device(self, scene: SceneBundle, width: int, height: int, ptrs: dict, after_stream=None, **kw):
        """Guide buffers into device memory (xrt_render_aov_device): ptrs maps plane names to
        device pointers (torch tensor .data_ptr()) of H*W*3 float32 (albedo, normal), H*W float32
        (depth, alpha) or H*W int32 (object); planes left out are not computed into.
        after_stream: the HIP stream whose queued work must finish before the buffers are
        overwritten (torch.cuda.current_stream().cuda_stream; None = the legacy default stream).
        Returns the stats when the planes are complete."""
        bad = [n for n in ptrs if n not in self._AOV_SHAPES]
        if bad:
            raise ValueError(f"unknown guide planes {bad}")
        if self._uploaded is not scene:
            self.upload(scene)
        p = self.params(scene, width, height, **kw)
        bufs = abi.XrtAovBuffers(**{n: int(v) for n, v in ptrs.items() if v})
        st = abi.XrtStats()
        self._check(self._lib.xrt_render_aov_device(self.ctx, C.byref(p), C.byref(bufs), C.c_void_p(after_stream or None),
                                                    C.byref(st)), "xrt_render_aov_device")
        self.stats = st
        return st

    def _filter_inputs(self, color, guides, width, height):
        """The filters' host inputs checked: (width, height, XrtAovBuffers over `guides`); the
        size is `color`'s when there is one."""
        bad = [n for n in guides if n not in self._AOV_SHAPES]
        if bad:
            raise ValueError(f"unknown guide planes {bad}")
        if color is not None:
            assert color.dtype == np.float32 and color.flags.c_contiguous and color.ndim == 3 and color.shape[2] == 3
            height, width = color.shape[:2]
        for n in abi.DENOISE_PLANES:
            a = guides.get(n)
            if a is not None:
                assert a.dtype == (np.int32 if n == "object" else np.float32) and a.flags.c_contiguous
                assert a.shape == (height, width) + self._AOV_SHAPES[n], n
        return width, height, abi.XrtAovBuffers(**{n: guides[n].ctypes.data for n in abi.DENOISE_PLANES
                                                   if guides.get(n) is not None})

    def _filter_inputs_device(self, guide_ptrs):
        """The XrtAovBuffers over a dict of device pointers, its names checked."""
        bad = [n for n in guide_ptrs if n not in self._AOV_SHAPES]
        if bad:
            raise ValueError(f"unknown guide planes {bad}")
        return abi.XrtAovBuffers(**{n: int(guide_ptrs[n]) for n in abi.DENOISE_PLANES if guide_ptrs.get(n)})

    @staticmethod
    def _denoise_params(width, height, iterations, sigma_color, sigma_normal, sigma_depth, sigma_albedo, tile, timing):
        return abi.XrtDenoiseParams(width, height, iterations, sigma_color, sigma_normal, sigma_depth, sigma_albedo,
                                    (abi.XRT_DENOISE_TIMING if timing else 0) | (0 if tile else abi.XRT_DENOISE_NO_TILE))

    def denoise(self, color, guides: dict, iterations=3, sigma_color=2.0, sigma_normal=0.5, sigma_depth=0.0,
                sigma_albedo=0.2, tile=True, timing=False, out=None, width=None, height=None) -> np.ndarray:
        """Edge-avoiding a-trous filter (xrt_denoise) of the (H, W, 3) float32 frame `color` over
        the guide planes of `guides` — albedo, normal, depth, object as render_aov returns them;
        alpha is accepted and not read, a plane left out (or None) counts as a plane of zeros.
        iterations passes with tap spacing 1, 2, 4, ...; a sigma <= 0 turns its term off.
        sigma_depth is the depth change tolerated per step of tap spacing in the scene's world
        units, so it has no scene-independent default and is off.  tile=False sends every
        iteration through the direct kernel (same results).  out: the (H, W, 3) float32 array to
        write (it may be `color`: in place); default a new one.  color=None filters the
        framebuffer of the last render(), whose size width and height then name.  Needs no
        scene.  The call's xrt_denoise_stats are left in self.denoise_stats."""
        width, height, bufs = self._filter_inputs(color, guides, width, height)
        if out is None:
            out = np.empty((height, width, 3), np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.shape == (height, width, 3)
        p = self._denoise_params(width, height, iterations, sigma_color, sigma_normal, sigma_depth, sigma_albedo, tile, timing)
        st = abi.XrtDenoiseStats()
        self._check(self._lib.xrt_denoise(self.ctx, C.byref(p), C.c_void_p(color.ctypes.data if color is not None else None),
                                          C.byref(bufs), C.c_void_p(out.ctypes.data), C.byref(st)), "xrt_denoise")
        self.denoise_stats = st
        return out

    def denoise_device(self, color_ptr, guide_ptrs: dict, out_ptr, width, height, after_stream=None, iterations=3,
                       sigma_color=2.0, sigma_normal=0.5, sigma_depth=0.0, sigma_albedo=0.2, tile=True, timing=False):
        """The filter over device memory (xrt_denoise_device): color_ptr and out_ptr are device
        pointers to H*W*3 float32 (they may be equal; color_ptr 0 = the last render's
        framebuffer), guide_ptrs maps plane names to device pointers laid out as
        render_aov_device writes them.  after_stream as for render_aov_device.  The settings
        are denoise()'s.  Returns the xrt_denoise_stats when out_ptr is complete."""
        bufs = self._filter_inputs_device(guide_ptrs)
        p = self._denoise_params(width, height, iterations, sigma_color, sigma_normal, sigma_depth, sigma_albedo, tile, timing)
        st = abi.XrtDenoiseStats()
        self._check(self._lib.xrt_denoise_device(self.ctx, C.byref(p), C.c_void_p(color_ptr or None), C.byref(bufs),
                                                 C.c_void_p(out_ptr or None), C.c_void_p(after_stream or None),
                                                 C.byref(st)), "xrt_denoise_device")
        self.denoise_stats = st
        return st

    @staticmethod
    def _denoise_var_params(width, height, iterations, sigma_luminance, sigma_normal, sigma_depth, sigma_albedo,
                            variance_radius, tile, timing):
        return abi.XrtDenoiseVarParams(width, height, iterations, sigma_luminance, sigma_normal, sigma_depth, sigma_albedo,
                                       variance_radius,
                                       (abi.XRT_DENOISE_TIMING if timing else 0) | (0 if tile else abi.XRT_DENOISE_NO_TILE))

    def denoise_var(self, color, guides: dict, variance=None, iterations=4, sigma_luminance=4.0, sigma_normal=0.5,
                    sigma_depth=0.0, sigma_albedo=0.2, variance_radius=3, tile=True, timing=False, out=None,
                    out_variance=None, want_variance=True, width=None, height=None):
        """Variance-guided a-trous filter (xrt_denoise_var, SVGF's spatial filter) of the (H, W, 3)
        float32 frame `color` over `guides` as denoise() takes them.  The colour stop is the
        luminance difference in units of sigma_luminance standard deviations of the centre
        pixel's noise, so it needs no tuning to the radiance scale.  variance: the (H, W) float32
        variance of each pixel's luminance (finite, >= 0); None: estimated from the frame over
        (2 variance_radius + 1)^2 pixels of the same object (variance_radius 1 .. 3).  out,
        out_variance: the arrays to write (they may be `color` and `variance`: in place);
        default new ones.  want_variance=False passes no variance output.  color=None, tile,
        timing, width, height as for denoise().  Returns (out, out_variance), out_variance None
        when not wanted; the call's xrt_denoise_stats are left in self.denoise_stats."""
        width, height, bufs = self._filter_inputs(color, guides, width, height)
        if variance is not None:
            assert variance.dtype == np.float32 and variance.flags.c_contiguous and variance.shape == (height, width)
        if out is None:
            out = np.empty((height, width, 3), np.float32)
        assert out.dtype == np.float32 and out.flags.c_contiguous and out.shape == (height, width, 3)
        if out_variance is None and want_variance:
            out_variance = np.empty((height, width), np.float32)
        if out_variance is not None:
            assert out_variance.dtype == np.float32 and out_variance.flags.c_contiguous and out_variance.shape == (height, width)
        p = self._denoise_var_params(width, height, iterations, sigma_luminance, sigma_normal, sigma_depth, sigma_albedo,
                                     variance_radius, tile, timing)
        st = abi.XrtDenoiseStats()
        self._check(self._lib.xrt_denoise_var(
            self.ctx, C.byref(p), C.c_void_p(color.ctypes.data if color is not None else None),
            C.c_void_p(variance.ctypes.data if variance is not None else None), C.byref(bufs), C.c_void_p(out.ctypes.data),
            C.c_void_p(out_variance.ctypes.data if out_variance is not None else None), C.byref(st)), "xrt_denoise_var")
        self.denoise_stats = st
        return out, out_variance

    def denoise_var_device(self, color_ptr, guide_ptrs: dict, out_ptr, width, height, variance_ptr=0, out_variance_ptr=0,
                           after_stream=None, iterations=4, sigma_luminance=4.0, sigma_normal=0.5, sigma_depth=0.0,
                           sigma_albedo=0.2, variance_radius=3, tile=True, timing=False):
        """The variance-guided filter over device memory (xrt_denoise_var_device): color_ptr, out_ptr
        and guide_ptrs as for denoise_device; variance_ptr and out_variance_ptr are device pointers
        to H*W float32 (they may be equal; variance_ptr 0 = estimate it, out_variance_ptr 0 = not
        wanted).  The settings are denoise_var()'s.  Returns the xrt_denoise_stats when the outputs
        are complete."""
        bufs = self._filter_inputs_device(guide_ptrs)
        p = self._denoise_var_params(width, height, iterations, sigma_luminance, sigma_normal, sigma_depth, sigma_albedo,
                                     variance_radius, tile, timing)
        st = abi.XrtDenoiseStats()
        self._check(self._lib.xrt_denoise_var_device(
            self.ctx, C.byref(p), C.c_void_p(color_ptr or None), C.c_void_p(variance_ptr or None), C.byref(bufs),
            C.c_void_p(out_ptr or None), C.c_void_p(out_variance_ptr or None), C.c_void_p(after_stream or None), C.byref(st)),
            "xrt_denoise_var_device")
        self.denoise_stats = st
        return st

    def query(self, scene: SceneBundle, rays: np.ndarray, tmax=None, occluded: bool = False):
        """Scene::intersect (or, with occluded=True, Scene::occluded(ray, tmax)) for rays
        (n, 6) = origin, direction, on the GPU with the render's trace kernels (xrt_query).
        Returns an array of abi.XrtHit."""
        if self._uploaded is not scene:
            self.upload(scene)
        r = np.ascontiguousarray(rays, dtype=np.float32).reshape(-1, 6)
        n = len(r)
        out = (abi.XrtHit * max(1, n))()
        tm = None if tmax is None else np.ascontiguousarray(np.broadcast_to(np.asarray(tmax, np.float32), (n,)))
        self._check(self._lib.xrt_query(self.ctx, n, abi.fptr(r), abi.fptr(tm) if tm is not None else None,
                                        abi.XRT_QUERY_OCCLUDED if occluded else abi.XRT_QUERY_INTERSECT, out),
                    "xrt_query")
        return out[:n]

    def camlist(self, scene: SceneBundle, width: int, height: int, shard_index: int = 0, shard_count: int = 1):
        """The camera lists the speculative merged schedule builds for the shard (xrt_test_camlist, a
        device self-test): (slots, 4) uint32 in pixel order, slot s = pixel s of the shard, whatever
        map a render uses — list bits 0-31, bits 32-63, the
        covering triangle or 0xffffffff, 0."""
        if self._uploaded is not scene:
            self.upload(scene)
        p = self.params(scene, width, height, shard_index=shard_index, shard_count=shard_count)
        out = np.zeros((len(range(shard_index, height, shard_count)) * width, 4), np.uint32)
        self._check(self._lib.xrt_test_camlist(self.ctx, C.byref(p), abi.u32ptr(out)), "xrt_test_camlist")
        return out

    def slot_map(self, scene: SceneBundle, width: int, height: int, **kw) -> np.ndarray:
        """The slot -> pixel map a render with these arguments (those of params) would use
        (xrt_test_slot_map, a device self-test): per slot of the shard its pixel index col + width * row."""
        if self._uploaded is not scene:
            self.upload(scene)
        p = self.params(scene, width, height, **kw)
        out = np.zeros(len(range(p.shard_index, height, p.shard_count)) * width, np.uint32)
        self._check(self._lib.xrt_test_slot_map(self.ctx, C.byref(p), abi.u32ptr(out)), "xrt_test_slot_map")
        return out

    def chunk_plan(self, scene: SceneBundle, width: int, height: int, **kw) -> dict:
        """The chunk phase a render with these arguments (those of params) would run (xrt_test_chunk_plan,
        a device self-test): {"chunks": bool, "passes", "C", "blocks", "sizes"}; sizes[c] are the live
        slots of chunk c = 8 j + class after the build, C counts the chunks that hold a slot."""
        if self._uploaded is not scene:
            self.upload(scene)
        p = self.params(scene, width, height, **kw)
        n = len(range(p.shard_index, height, p.shard_count)) * width
        sizes = np.zeros(8 * (n // 256 + 2), np.uint32)   # chunks are numbered 8 j + class: one class may hold them all
        plan = np.zeros(5, np.uint32)
        self._check(self._lib.xrt_test_chunk_plan(self.ctx, C.byref(p), abi.u32ptr(plan), abi.u32ptr(sizes), len(sizes)),
                    "xrt_test_chunk_plan")
        return dict(chunks=bool(plan[0]), passes=int(plan[1]), C=int(plan[2]), blocks=int(plan[3]),
                    sizes=sizes[:min(len(sizes), int(plan[4]))].copy())

    def tonemap(self, width: int, height: int, gamma: float, device_ptr: int = 0) -> np.ndarray:
        """Image::gammaCorrection(gamma) + writePPM's 8-bit quantisation on the GPU, of the
        last render() (device_ptr 0) or of a device float3 buffer: (H, W, 3) uint8."""
        out = np.empty((height, width, 3), np.uint8)
        self._check(self._lib.xrt_tonemap(self.ctx, C.c_void_p(device_ptr or None), width * height, C.c_float(gamma),
                                          out.ctypes.data_as(C.POINTER(C.c_uint8))), "xrt_tonemap")
        return out

    @staticmethod
    def write_ppm(path: str, rgb8: np.ndarray):
        """Image::writePPM's text format (Src/image.h:92-114): P3, width height, 255, one
        "R G B" line per pixel."""
        h, w, _ = rgb8.shape
        with open(path, "w") as f:
            f.write(f"P3\n{w} {h}\n255\n")
            f.write("".join(f"{r} {g} {b}\n" for r, g, b in rgb8.reshape(-1, 3).tolist()))

    def render_device(self, scene: SceneBundle, width: int, height: int, out_ptr: int, after_stream=None, **kw):
        """Render into a device buffer (e.g. torch tensor .data_ptr()) of H*W*3 float32.
        after_stream: a HIP stream handle (torch.cuda.current_stream().cuda_stream) whose
        queued work must finish before the buffer is overwritten; None = wait for the whole
        device.  Returns when the image is complete."""
        if self._uploaded is not scene:
            self.upload(scene)
        p = self.params(scene, width, height, **kw)
        st = abi.XrtStats()
        if after_stream is None:
            rc = self._lib.xrt_render_device(self.ctx, C.byref(p), C.c_void_p(out_ptr), C.byref(st))
        else:
            rc = self._lib.xrt_render_device_after(self.ctx, C.byref(p), C.c_void_p(out_ptr),
                                                   C.c_void_p(after_stream or None), C.byref(st))
        self._check(rc, "xrt_render_device")
        self.stats = st
        return st
