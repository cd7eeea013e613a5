"""The edge-avoiding a-trous filter on the GPU (xrt_denoise, denoise.hip) against the restatement
(tests/denoise_restatement.py): every frame bit for bit, under the default path and under
XRT_DENOISE_NO_TILE.  The cases and the situations they are chosen for are in
tests/denoise_restatement.py and checked without a GPU in tests/test_denoise_restatement.py."""
import ctypes as C

import numpy as np
import pytest

import aov_restatement as ar
import denoise_restatement as dr
import pyoracle
from gpu_checks import assert_same_bits, read_ppm, run_example, words
from gpu_checks import renderer as r  # noqa: F401 -- the shared fixture, under the name the tests here ask for
from xraytracer_amd import abi, scenes
from xraytracer_amd.renderer import HipRenderer

pytestmark = pytest.mark.gpu


def check_stats(st, iterations, tile):
    tiled = min(iterations, abi.XRT_DENOISE_TILED_ITERATIONS) if tile else 0
    assert (st.tiled_iterations, st.direct_iterations) == (tiled, iterations - tiled)
    assert st.launches == iterations + 1 and st.reserved == 0


# 1. every case, through both kernels
@pytest.mark.parametrize("tile", [True, False])
@pytest.mark.parametrize("name", sorted(dr.CASES))
def test_cases(r, name, tile):
    color, g = dr.inputs(name)
    kw = dr.CASES[name][3]
    got = r.denoise(color, g, tile=tile, **kw)
    check_stats(r.denoise_stats, kw["iterations"], tile)
    assert_same_bits(got, dr.reference(name)[0])


# 2. guide-plane subsets: a plane left out is a plane of zeros
@pytest.mark.parametrize("subset", [(), ("normal",), ("depth", "object"), dr.GUIDES])
def test_plane_subsets(r, subset):
    color, g = dr.inputs("synthetic_3")
    kw = dr.CASES["synthetic_3"][3]
    sub = {k: g[k] for k in subset}
    ref = dr.denoise(color, sub, **kw)
    for tile in (True, False):
        assert_same_bits(r.denoise(color, sub, tile=tile, **kw), ref)
    if not subset:   # a NULL guides struct through the C call
        out = np.empty_like(ref)
        p = abi.XrtDenoiseParams(color.shape[1], color.shape[0], kw["iterations"], kw["sigma_color"], kw["sigma_normal"],
                                 kw["sigma_depth"], kw["sigma_albedo"], 0)
        assert abi.lib().xrt_denoise(r.ctx, C.byref(p), color.ctypes.data, None, out.ctypes.data, None) == 0
        assert_same_bits(out, ref)


# 3. a sigma <= 0 equals that plane being NULL
@pytest.mark.parametrize("plane,sigma", [("albedo", "sigma_albedo"), ("normal", "sigma_normal"), ("depth", "sigma_depth")])
def test_sigma_off_equals_null_plane(r, plane, sigma):
    color, g = dr.inputs("synthetic_2")
    kw = dr.CASES["synthetic_2"][3]
    without = r.denoise(color, {k: v for k, v in g.items() if k != plane}, **kw)
    for off in (0.0, -1.0):
        assert_same_bits(r.denoise(color, g, **dict(kw, **{sigma: off})), without)
    # sigma_color off: the restatement's frame
    off = dict(kw, sigma_color=0.0)
    assert_same_bits(r.denoise(color, g, **off), dr.denoise(color, g, **off))


# 4. in place
@pytest.mark.parametrize("tile", [True, False])
def test_in_place(r, tile):
    color, g = dr.inputs("130x70")
    kw = dr.CASES["130x70"][3]
    buf = np.array(color)
    assert r.denoise(buf, g, out=buf, tile=tile, **kw) is buf
    assert_same_bits(buf, dr.reference("130x70")[0])


# 5. the device entry point: torch tensors written on the current stream right before the call, guard
#    words round the output, in and out of place, on one device and on a two-entry context
@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_device_entry_point(devices):
    import torch

    name = "130x70"
    color, g = dr.inputs(name)
    kw = dr.CASES[name][3]
    ref = dr.reference(name)[0]
    h, w = color.shape[:2]
    n, pad = 3 * w * h, 64
    dev = "cuda:0"
    hr = HipRenderer(1, devices=devices)
    try:
        for in_place in (False, True):
            stream = torch.cuda.current_stream().cuda_stream
            t = {k: torch.empty(v.shape, dtype=torch.int32 if k == "object" else torch.float32, device=dev) for k, v in g.items()}
            out = torch.empty(pad + n + pad, dtype=torch.float32, device=dev)
            src = torch.empty(n, dtype=torch.float32, device=dev)
            # queued on the current stream, not waited for: the filter must order itself behind them
            for k, v in g.items():
                t[k].copy_(torch.from_numpy(np.array(v)), non_blocking=True)
            out.fill_(-7.0)
            host_color = torch.from_numpy(np.array(color).reshape(-1))
            (out[pad:pad + n] if in_place else src).copy_(host_color, non_blocking=True)
            out_ptr = out.data_ptr() + 4 * pad
            st = hr.denoise_device(out_ptr if in_place else src.data_ptr(), {k: v.data_ptr() for k, v in t.items()}, out_ptr,
                                   w, h, after_stream=stream, **kw)
            check_stats(st, kw["iterations"], True)
            torch.cuda.synchronize()
            got = out.cpu().numpy()
            assert (got[:pad] == -7.0).all() and (got[pad + n:] == -7.0).all()
            assert_same_bits(got[pad:pad + n].reshape(h, w, 3), ref)
            if not in_place:
                assert np.array_equal(src.cpu().numpy(), np.array(color).reshape(-1))   # the input is only read
    finally:
        hr.close()


# 6. color = NULL: the framebuffer of the last xrt_render
@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_null_color_is_the_last_render(devices):
    w, h = 24, 18
    s = scenes.cornell(w, h)
    hr = HipRenderer(2, devices=devices)
    try:
        p = abi.XrtDenoiseParams(w, h, 2, 2.0, 0.0, 0.0, 0.0, 0)
        out = np.zeros((h, w, 3), np.float32)
        assert abi.lib().xrt_denoise(hr.ctx, C.byref(p), None, None, out.ctypes.data, None) == abi.XRT_ERR_STATE
        assert abi.lib().xrt_denoise_device(hr.ctx, C.byref(p), None, None, out.ctypes.data, None, None) == abi.XRT_ERR_STATE
        frame = hr.render(s, w, h)
        guides = hr.render_aov(s, w, h, planes=dr.GUIDES)
        kw = dict(iterations=2, sigma_depth=32.0)
        from_fb = hr.denoise(None, guides, width=w, height=h, **kw)
        assert_same_bits(from_fb, hr.denoise(frame, guides, **kw))
        assert_same_bits(from_fb, dr.denoise(frame, guides, **dict(dr.DEFAULTS, **kw)))
        # a frame larger than the framebuffer is refused
        p = abi.XrtDenoiseParams(4 * w, 4 * h, 1, 2.0, 0.0, 0.0, 0.0, 0)
        big = np.zeros((4 * h, 4 * w, 3), np.float32)
        assert abi.lib().xrt_denoise(hr.ctx, C.byref(p), None, None, big.ctypes.data, None) == abi.XRT_ERR_STATE
    finally:
        hr.close()


# 7. refusals
def test_invalid_arguments(r):
    lib = abi.lib()
    buf = np.zeros((4, 4, 3), np.float32)
    ptr = buf.ctypes.data

    def rc(params, out=ptr, ctx=r.ctx):
        return lib.xrt_denoise(ctx, C.byref(params) if params is not None else None, ptr, None, out, None)

    ok = abi.XrtDenoiseParams(4, 4, 1, 1.0, 1.0, 1.0, 1.0, 0)
    assert rc(ok) == 0
    assert rc(ok, ctx=None) == abi.XRT_ERR_INVALID
    assert rc(None) == abi.XRT_ERR_INVALID
    assert rc(ok, out=None) == abi.XRT_ERR_INVALID
    assert lib.xrt_denoise_device(r.ctx, C.byref(ok), None, None, None, None, None) == abi.XRT_ERR_INVALID
    for width, height, iterations in ((0, 4, 1), (4, 0, 1), (4, 4, 0), (4, 4, abi.XRT_DENOISE_MAX_ITERATIONS + 1)):
        assert rc(abi.XrtDenoiseParams(width, height, iterations, 1.0, 1.0, 1.0, 1.0, 0)) == abi.XRT_ERR_INVALID
    assert lib.xrt_last_error(r.ctx)
    with pytest.raises(ValueError):
        r.denoise(buf, dict(colour=buf))
    with pytest.raises(ValueError):
        r.denoise_device(1, dict(nrm=1), 1, 4, 4)


# 8. the timing flag
def test_timing_flag(r):
    color, g = dr.inputs("synthetic_3")
    kw = dr.CASES["synthetic_3"][3]
    r.denoise(color, g, timing=True, **kw)
    assert r.denoise_stats.kernel_ms > 0 and r.denoise_stats.wall_ms > 0
    r.denoise(color, g, **kw)
    assert r.denoise_stats.kernel_ms == 0 and r.denoise_stats.wall_ms > 0


# 9. end to end: a GPU GI render, its guide buffers and the filter, against the restatement applied to
#    those same GPU outputs
def test_render_guides_denoise():
    w, h, spp = 64, 48, 16
    s = scenes.cornell(w, h)
    hr = HipRenderer(spp)
    try:
        frame = hr.render(s, w, h)
        guides = hr.render_aov(s, w, h)
        kw = dict(iterations=2, sigma_color=2.0, sigma_normal=0.5, sigma_depth=32.0, sigma_albedo=0.2)
        got = hr.denoise(frame, guides, **kw)
    finally:
        hr.close()
    assert_same_bits(got, dr.denoise(frame, guides, **kw))
    assert not np.array_equal(words(got), words(frame))


# 10. examples/denoise.cpp through the C++ API (HipRenderer::denoise)
def example_scene(w, h):
    """examples/denoise.cpp: the example's plane and sphere under a QuadLight, GIIntegrator(3)"""
    s = scenes.SceneBundle()
    s.add_mesh("plane", scenes.EXAMPLE_PLANE, (1.0, 1.0, 1.0))
    s.add_sphere("sphere_diffuse", (0.0, 0.0, 0.0), 1.0, (0.58, 0.58, 0.58))
    s.add_quad_light("QuadLight", (1.0, 4.0, -1.0), (1.0, 4.0, 1.0), (-1.0, 4.0, -1.0), (25.0, 25.0, 25.0))
    s.flatten()
    s.camera = scenes.pinhole((1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 8, 1), 60.0, w, h)
    s.integrator, s.max_depth = "gi", 3
    return s


def test_denoise_example_ppm(tmp_path):
    w, h, spp = 48, 36, 4
    prefix = tmp_path / "frame"
    run_example("denoise", w, h, spp, prefix)
    s = example_scene(w, h)
    frame, _ = pyoracle.render(s, w, h, spp)
    planes, _, _ = ar.render(s, w, h, spp)
    assert frame.max() > 0
    assert np.array_equal(read_ppm(tmp_path / "frame.noisy.ppm", w, h), pyoracle.tonemap(frame, 1.2).astype(np.int64))
    want = dr.denoise(frame, planes, **dr.DEFAULTS)
    assert np.array_equal(read_ppm(tmp_path / "frame.denoised.ppm", w, h), pyoracle.tonemap(want, 1.2).astype(np.int64))
