"""The variance-guided a-trous filter on the GPU (xrt_denoise_var, denoise.hip) against the
restatement (tests/denoise_var_restatement.py): every frame and the variance left bit for bit, under
the default path and under XRT_DENOISE_NO_TILE.  The cases and the situations they are chosen for
are in tests/denoise_var_restatement.py and checked without a GPU in
tests/test_denoise_var_restatement.py."""
import ctypes as C

import numpy as np
import pytest

import aov_restatement as ar
import denoise_restatement as dr
import denoise_var_restatement as dv
import pyoracle
from gpu_checks import assert_same_bits, read_ppm, run_example, words
from gpu_checks import renderer as r  # noqa: F401 -- the shared fixture, under the name the tests here ask for
from xraytracer_amd import abi, scenes
from xraytracer_amd.renderer import HipRenderer

pytestmark = pytest.mark.gpu


def check_stats(st, iterations, tile, estimated):
    tiled = min(iterations, abi.XRT_DENOISE_VAR_TILED_ITERATIONS) if tile else 0
    assert (st.tiled_iterations, st.direct_iterations) == (tiled, iterations - tiled)
    assert st.launches == iterations + 1 + (1 if estimated else 0) and st.reserved == 0


# 1. every case, through both kernels
@pytest.mark.parametrize("tile", [True, False])
@pytest.mark.parametrize("name", sorted(dv.CASES))
def test_cases(r, name, tile):
    color, g, variance = dv.inputs(name)
    kw = dv.CASES[name][4]
    got, var = r.denoise_var(color, g, variance, tile=tile, **kw)
    check_stats(r.denoise_stats, kw["iterations"], tile, variance is None)
    ref, ref_var, _ = dv.reference(name)
    assert_same_bits(got, ref)
    assert_same_bits(var, ref_var)


# 2. the estimate fed back as the caller's variance gives the bits of variance = NULL
@pytest.mark.parametrize("name", ["synthetic_3", "synthetic_r1_3", "130x70"])
def test_estimate_equals_supplied_estimate(r, name):
    color, g, _ = dv.inputs(name)
    kw = dv.CASES[name][4]
    est = dv.estimate(color, g["object"], kw["variance_radius"])
    for tile in (True, False):
        got, var = r.denoise_var(color, g, est, tile=tile, **kw)
        check_stats(r.denoise_stats, kw["iterations"], tile, False)
        assert_same_bits(got, dv.reference(name)[0])
        assert_same_bits(var, dv.reference(name)[1])


# 3. guide-plane subsets: a plane left out is a plane of zeros
@pytest.mark.parametrize("subset", [(), ("normal",), ("depth", "object"), dr.GUIDES])
def test_plane_subsets(r, subset):
    color, g, _ = dv.inputs("synthetic_3")
    kw = dv.CASES["synthetic_3"][4]
    sub = {k: g[k] for k in subset}
    ref, ref_var = dv.denoise_var(color, sub, None, **kw)
    for tile in (True, False):
        got, var = r.denoise_var(color, sub, tile=tile, **kw)
        assert_same_bits(got, ref)
        assert_same_bits(var, ref_var)
    if not subset:   # a NULL guides struct through the C call
        out, outv = np.empty_like(ref), np.empty_like(ref_var)
        p = abi.XrtDenoiseVarParams(color.shape[1], color.shape[0], kw["iterations"], kw["sigma_luminance"], kw["sigma_normal"],
                                    kw["sigma_depth"], kw["sigma_albedo"], kw["variance_radius"], 0)
        assert abi.lib().xrt_denoise_var(r.ctx, C.byref(p), color.ctypes.data, None, None, out.ctypes.data, outv.ctypes.data,
                                         None) == 0
        assert_same_bits(out, ref)
        assert_same_bits(outv, ref_var)


# 4. each sigma <= 0: the guide sigmas equal that plane being NULL, sigma_luminance the restatement's
#    frame, which is xrt_denoise's with sigma_color = 0
@pytest.mark.parametrize("plane,sigma", [("albedo", "sigma_albedo"), ("normal", "sigma_normal"), ("depth", "sigma_depth")])
def test_sigma_off_equals_null_plane(r, plane, sigma):
    color, g, _ = dv.inputs("synthetic_2")
    kw = dv.CASES["synthetic_2"][4]
    without = r.denoise_var(color, {k: v for k, v in g.items() if k != plane}, **kw)
    for off in (0.0, -1.0):
        got = r.denoise_var(color, g, **dict(kw, **{sigma: off}))
        assert_same_bits(got[0], without[0])
        assert_same_bits(got[1], without[1])


def test_sigma_luminance_off(r):
    color, g, _ = dv.inputs("synthetic_3")
    kw = dv.CASES["synthetic_3"][4]
    plain = r.denoise(color, g, iterations=kw["iterations"], sigma_color=0.0, sigma_normal=kw["sigma_normal"],
                      sigma_depth=kw["sigma_depth"], sigma_albedo=kw["sigma_albedo"])
    for off in (0.0, -1.0):
        o = dict(kw, sigma_luminance=off)
        ref, ref_var = dv.denoise_var(color, g, None, **o)
        for tile in (True, False):
            got, var = r.denoise_var(color, g, tile=tile, **o)
            assert_same_bits(got, ref)
            assert_same_bits(var, ref_var)
            assert_same_bits(got, plain)


# 5. out_variance NULL
def test_no_variance_output(r):
    color, g, variance = dv.inputs("supplied")
    kw = dv.CASES["supplied"][4]
    got, var = r.denoise_var(color, g, variance, want_variance=False, **kw)
    assert var is None
    assert_same_bits(got, dv.reference("supplied")[0])


# 6. in place, for both colour and variance
@pytest.mark.parametrize("tile", [True, False])
def test_in_place(r, tile):
    color, g, variance = dv.inputs("supplied")
    kw = dv.CASES["supplied"][4]
    buf, vbuf = np.array(color), np.array(variance)
    got = r.denoise_var(buf, g, vbuf, out=buf, out_variance=vbuf, tile=tile, **kw)
    assert got[0] is buf and got[1] is vbuf
    assert_same_bits(buf, dv.reference("supplied")[0])
    assert_same_bits(vbuf, dv.reference("supplied")[1])
    color, g, _ = dv.inputs("130x70")
    buf = np.array(color)
    got = r.denoise_var(buf, g, out=buf, tile=tile, **dv.CASES["130x70"][4])
    assert_same_bits(buf, dv.reference("130x70")[0])
    assert_same_bits(got[1], dv.reference("130x70")[1])


# 7. the device entry point: torch tensors written on the current stream right before the call, guard
#    words round both outputs, in and out of place, with a caller's variance and with the estimate, on
#    one device and on a two-entry context
@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_device_entry_point(devices):
    import torch

    dev, pad = "cuda:0", 64
    hr = HipRenderer(1, devices=devices)
    try:
        for name, in_place in (("supplied", False), ("supplied", True), ("130x70", False)):
            color, g, variance = dv.inputs(name)
            kw = dv.CASES[name][4]
            ref, ref_var, _ = dv.reference(name)
            h, w = color.shape[:2]
            n, nv = 3 * w * h, w * h
            stream = torch.cuda.current_stream().cuda_stream
            t = {k: torch.empty(v.shape, dtype=torch.int32 if k == "object" else torch.float32, device=dev) for k, v in g.items()}
            out = torch.empty(pad + n + pad, dtype=torch.float32, device=dev)
            outv = torch.empty(pad + nv + pad, dtype=torch.float32, device=dev)
            src = torch.empty(n, dtype=torch.float32, device=dev)
            srcv = torch.empty(nv, dtype=torch.float32, device=dev)
            # queued on the current stream, not waited for: the filter must order itself behind them
            for k, v in g.items():
                t[k].copy_(torch.from_numpy(np.array(v)), non_blocking=True)
            out.fill_(-7.0)
            outv.fill_(-7.0)
            (out[pad:pad + n] if in_place else src).copy_(torch.from_numpy(np.array(color).reshape(-1)), non_blocking=True)
            if variance is not None:
                (outv[pad:pad + nv] if in_place else srcv).copy_(torch.from_numpy(np.array(variance).reshape(-1)), non_blocking=True)
            out_ptr, outv_ptr = out.data_ptr() + 4 * pad, outv.data_ptr() + 4 * pad
            var_ptr = 0 if variance is None else (outv_ptr if in_place else srcv.data_ptr())
            st = hr.denoise_var_device(out_ptr if in_place else src.data_ptr(), {k: v.data_ptr() for k, v in t.items()}, out_ptr,
                                       w, h, variance_ptr=var_ptr, out_variance_ptr=outv_ptr, after_stream=stream, **kw)
            check_stats(st, kw["iterations"], True, variance is None)
            torch.cuda.synchronize()
            got, gotv = out.cpu().numpy(), outv.cpu().numpy()
            assert (got[:pad] == -7.0).all() and (got[pad + n:] == -7.0).all()
            assert (gotv[:pad] == -7.0).all() and (gotv[pad + nv:] == -7.0).all()
            assert_same_bits(got[pad:pad + n].reshape(h, w, 3), ref)
            assert_same_bits(gotv[pad:pad + nv].reshape(h, w), ref_var)
            if not in_place:   # the inputs are only read
                assert np.array_equal(src.cpu().numpy(), np.array(color).reshape(-1))
                if variance is not None:
                    assert np.array_equal(srcv.cpu().numpy(), np.array(variance).reshape(-1))
    finally:
        hr.close()


# 8. color = NULL: the framebuffer of the last xrt_render
@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_null_color_is_the_last_render(devices):
    w, h = 24, 18
    s = scenes.cornell(w, h)
    hr = HipRenderer(2, devices=devices)
    try:
        p = abi.XrtDenoiseVarParams(w, h, 2, 4.0, 0.0, 0.0, 0.0, 2, 0)
        out = np.zeros((h, w, 3), np.float32)
        lib = abi.lib()
        assert lib.xrt_denoise_var(hr.ctx, C.byref(p), None, None, None, out.ctypes.data, None, None) == abi.XRT_ERR_STATE
        assert lib.xrt_denoise_var_device(hr.ctx, C.byref(p), None, None, None, out.ctypes.data, None, None, None) == abi.XRT_ERR_STATE
        frame = hr.render(s, w, h)
        guides = hr.render_aov(s, w, h, planes=dr.GUIDES)
        kw = dict(iterations=2, sigma_depth=32.0, variance_radius=2)
        from_fb = hr.denoise_var(None, guides, width=w, height=h, **kw)
        direct = hr.denoise_var(frame, guides, **kw)
        ref = dv.denoise_var(frame, guides, None, **dict(dv.DEFAULTS, **kw))
        for k in (0, 1):
            assert_same_bits(from_fb[k], direct[k])
            assert_same_bits(from_fb[k], ref[k])
        # a frame larger than the framebuffer is refused
        p = abi.XrtDenoiseVarParams(4 * w, 4 * h, 1, 4.0, 0.0, 0.0, 0.0, 2, 0)
        big = np.zeros((4 * h, 4 * w, 3), np.float32)
        assert lib.xrt_denoise_var(hr.ctx, C.byref(p), None, None, None, big.ctypes.data, None, None) == abi.XRT_ERR_STATE
    finally:
        hr.close()


# 9. refusals
def test_invalid_arguments(r):
    lib = abi.lib()
    buf = np.zeros((4, 4, 3), np.float32)
    var = np.zeros((4, 4), np.float32)
    ptr = buf.ctypes.data

    def rc(params, out=ptr, ctx=r.ctx, variance=None):
        return lib.xrt_denoise_var(ctx, C.byref(params) if params is not None else None, ptr, variance, None, out, None, None)

    ok = abi.XrtDenoiseVarParams(4, 4, 1, 4.0, 1.0, 1.0, 1.0, 3, 0)
    assert rc(ok) == 0
    assert rc(ok, ctx=None) == abi.XRT_ERR_INVALID
    assert rc(None) == abi.XRT_ERR_INVALID
    assert rc(ok, out=None) == abi.XRT_ERR_INVALID
    assert lib.xrt_denoise_var_device(r.ctx, C.byref(ok), None, None, None, None, None, None, None) == abi.XRT_ERR_INVALID
    for width, height, iterations in ((0, 4, 1), (4, 0, 1), (4, 4, 0), (4, 4, abi.XRT_DENOISE_MAX_ITERATIONS + 1)):
        assert rc(abi.XrtDenoiseVarParams(width, height, iterations, 4.0, 1.0, 1.0, 1.0, 3, 0)) == abi.XRT_ERR_INVALID
    # variance_radius: 1 .. 3 while the library estimates, not read with a caller's variance
    for radius in (0, abi.XRT_DENOISE_VAR_MAX_RADIUS + 1, 1 << 31):
        bad = abi.XrtDenoiseVarParams(4, 4, 1, 4.0, 1.0, 1.0, 1.0, radius, 0)
        assert rc(bad) == abi.XRT_ERR_INVALID
        assert lib.xrt_last_error(r.ctx)
        assert rc(bad, variance=var.ctypes.data) == 0
    for radius in (1, 2, 3):
        assert rc(abi.XrtDenoiseVarParams(4, 4, 1, 4.0, 1.0, 1.0, 1.0, radius, 0)) == 0
    with pytest.raises(ValueError):
        r.denoise_var(buf, dict(colour=buf))
    with pytest.raises(ValueError):
        r.denoise_var_device(1, dict(nrm=1), 1, 4, 4)


# 10. the timing flag
def test_timing_flag(r):
    color, g, _ = dv.inputs("synthetic_3")
    kw = dv.CASES["synthetic_3"][4]
    r.denoise_var(color, g, timing=True, **kw)
    assert r.denoise_stats.kernel_ms > 0 and r.denoise_stats.wall_ms > 0
    r.denoise_var(color, g, **kw)
    assert r.denoise_stats.kernel_ms == 0 and r.denoise_stats.wall_ms > 0


# 11. the two filters share the context's records and staging: neither sees what the other left.  The
#     larger frame goes first, so each later call runs in a buffer that still holds the other
#     filter's larger records.
def test_filters_alternate_in_one_context():
    plain_color, plain_g = dr.inputs("synthetic_3")   # 37 x 29
    plain_kw = dr.CASES["synthetic_3"][3]
    hr = HipRenderer(1)
    try:
        for tile in (True, False):
            plain = []
            for name in ("130x70", "supplied"):
                color, g, variance = dv.inputs(name)
                got, var = hr.denoise_var(color, g, variance, tile=tile, **dv.CASES[name][4])
                assert_same_bits(got, dv.reference(name)[0])
                assert_same_bits(var, dv.reference(name)[1])
                plain.append(hr.denoise(plain_color, plain_g, tile=tile, **plain_kw))
                assert_same_bits(plain[-1], dr.reference("synthetic_3")[0])
            assert_same_bits(plain[0], plain[1])
    finally:
        hr.close()


# 12. end to end: a GPU GI render, its guide buffers and the filter, against the restatement applied to
#     those same GPU outputs
def test_render_guides_denoise_var():
    w, h, spp = 64, 48, 16
    s = scenes.cornell(w, h)
    hr = HipRenderer(spp)
    try:
        frame = hr.render(s, w, h)
        guides = hr.render_aov(s, w, h)
        kw = dict(iterations=4, sigma_luminance=4.0, sigma_normal=0.5, sigma_depth=32.0, sigma_albedo=0.2, variance_radius=3)
        got, var = hr.denoise_var(frame, guides, **kw)
    finally:
        hr.close()
    ref, ref_var = dv.denoise_var(frame, guides, None, **kw)
    assert_same_bits(got, ref)
    assert_same_bits(var, ref_var)
    assert not np.array_equal(words(got), words(frame))


# 12. examples/denoise_var.cpp through the C++ API (HipRenderer::denoiseVar)
def test_denoise_var_example_ppm(tmp_path):
    w, h, spp = 48, 36, 4
    prefix = tmp_path / "frame"
    run_example("denoise_var", w, h, spp, prefix)
    # examples/denoise.cpp's scene: the example's plane and sphere under a QuadLight, GIIntegrator(3)
    s = scenes.SceneBundle()
    s.add_mesh("plane", scenes.EXAMPLE_PLANE, (1.0, 1.0, 1.0))
    s.add_sphere("sphere_diffuse", (0.0, 0.0, 0.0), 1.0, (0.58, 0.58, 0.58))
    s.add_quad_light("QuadLight", (1.0, 4.0, -1.0), (1.0, 4.0, 1.0), (-1.0, 4.0, -1.0), (25.0, 25.0, 25.0))
    s.flatten()
    s.camera = scenes.pinhole((1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 8, 1), 60.0, w, h)
    s.integrator, s.max_depth = "gi", 3
    frame, _ = pyoracle.render(s, w, h, spp)
    planes, _, _ = ar.render(s, w, h, spp)
    assert frame.max() > 0
    assert np.array_equal(read_ppm(tmp_path / "frame.noisy.ppm", w, h), pyoracle.tonemap(frame, 1.2).astype(np.int64))
    want, _ = dv.denoise_var(frame, planes, None, **dv.DEFAULTS)
    assert np.array_equal(read_ppm(tmp_path / "frame.denoised.ppm", w, h), pyoracle.tonemap(want, 1.2).astype(np.int64))
