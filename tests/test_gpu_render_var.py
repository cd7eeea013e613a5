"""xrt_render_var on the GPU (the moments builds of k_shade, k_whitted and k_whitted_bvh, and
k_finish_var) against the restatement (tests/render_var_restatement.py): the frame bit for bit the
oracle's and xrt_render's, the variance plane bit for bit the restatement's, the counters the
oracle's, the schedule the contract's.  The cases and the situations they are chosen for are in
tests/render_var_restatement.py and checked without a GPU in tests/test_render_var_restatement.py."""
import ctypes as C

import numpy as np
import pytest

import aov_restatement as ar
import denoise_restatement as dr
import denoise_var_restatement as dv
import pyoracle
import render_var_restatement as rv
import whitted_scenes as ws
from gpu_checks import assert_frame, assert_same_bits, counters_equal, read_ppm, run_example
from xraytracer_amd import abi, scenes
from xraytracer_amd.renderer import HipRenderer

pytestmark = pytest.mark.gpu

# xrt_stats fields that do not depend on how far the host ran ahead of the termination polls
STABLE = ("samples", "segments", "shadow_rays", "draws", "rejected", "path_slots", "schedule", "stalled", "slots_per_wave",
          "group_lanes", "partitions", "visits_per_launch", "rng_twists", "pix_windows", "pix_flushes", "spec_launches",
          "whit_rays", "whit_depth_cut", "whit_refract", "whit_tir")


@pytest.fixture(scope="module")
def hr():
    r = HipRenderer(2, device=0)
    yield r
    r.close()


def stable(st):
    return {k: int(getattr(st, k)) for k in STABLE}


def render_kw(name):
    kw = dict(rv.CASES[name][4])
    if name in rv.WHITTED_BVH:
        kw["whitted_bvh"] = True
    return kw


def check_case(hr, name, sched=abi.XRT_SCHED_WAVEFRONT, **extra):
    """CASES[name] through xrt_render_var: frame, plane, counters and schedule; returns the stats"""
    _, w, h, spp, _ = rv.CASES[name]
    kw = render_kw(name)
    hr.spp = spp
    hr._uploaded = None
    img, var = hr.render_var(rv.scene(name), w, h, **kw, **extra)
    st = hr.stats
    ref, cnt = rv.oracle_frame(name)
    assert st.schedule == sched
    assert_frame(img, ref)
    assert_same_bits(var, rv.reference(name)[1], name)
    if kw.get("integrator") == "whitted":
        assert {k: int(getattr(st, k)) for k in ws.COUNTERS} == {k: int(cnt[k]) for k in ws.COUNTERS}
    else:
        counters_equal(st, cnt)
    return img, var, st


def check_against_render(hr, name, img, st):
    """the frame is xrt_render's at its default schedule on the same context, and the stats are
    xrt_render's under XRT_FLAG_WAVEFRONT"""
    _, w, h, _, _ = rv.CASES[name]
    kw = render_kw(name)
    assert_frame(hr.render(rv.scene(name), w, h, **kw), img)
    assert_frame(hr.render(rv.scene(name), w, h, schedule="wavefront", **kw), img)
    assert stable(hr.stats) == stable(st)


# 1. the six path integrators
@pytest.mark.parametrize("name", ["gi", "direct", "indirect", "normal", "vpt_smoke", "vpt_nee_smoke", "vpt_homogeneous",
                                  "vpt_nee_homogeneous"])
def test_integrators(hr, name):
    img, _, st = check_case(hr, name)
    check_against_render(hr, name, img, st)


# 2. the scene families: a sphere BVH, mixed scenes, a two-level scene, rings twisted several times
@pytest.mark.parametrize("name", ["spheres", "example", "mixed_lit", "two_level", "twists"])
def test_scene_families(hr, name):
    img, _, st = check_case(hr, name)
    check_against_render(hr, name, img, st)
    if name == "twists":
        assert st.rng_twists > st.path_slots
    if name == "two_level":
        assert st.launches[abi.XRT_K_DEEP] > 0


# 3. rejected samples add nothing to either plane
@pytest.mark.parametrize("name", ["rejects_gi", "rejects_direct"])
def test_rejects(hr, name):
    img, _, st = check_case(hr, name)
    assert st.rejected > 1000
    check_against_render(hr, name, img, st)


# 4. WhittedIntegrator, round the edges of the 64-sample window
@pytest.mark.parametrize("name", sorted(n for n in rv.CASES if n.startswith("whitted")))
def test_whitted(hr, name):
    bvh = name in rv.WHITTED_BVH
    img, _, st = check_case(hr, name, abi.XRT_SCHED_WHITTED_BVH if bvh else abi.XRT_SCHED_WHITTED)
    if name == "whitted_rejects_65":
        assert st.rejected > 0
    check_against_render(hr, name, img, st)


# 5. shards
def test_shard_leaves_other_rows_zero(hr):
    img, var, st = check_case(hr, "shard")
    rows = np.arange(12) % 3 == 1
    assert not img.view(np.uint32)[~rows].any() and not var.view(np.uint32)[~rows].any()
    assert st.samples == 4 * 16 * 4


def test_shard_without_rows(hr):
    s = scenes.cornell(8, 2)
    hr.spp = 2
    img, var = hr.render_var(s, 8, 2, shard_index=3, shard_count=4)
    assert not img.view(np.uint32).any() and not var.view(np.uint32).any()
    assert hr.stats.samples == 0


# 6. the device entry point: torch tensors written on the current stream right before the call, guard
#    words round both outputs, on one device and on a two-entry context; the context's last
#    framebuffer is this frame afterwards
@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_device_entry_point(devices):
    import torch

    dev, pad = "cuda:0", 64
    r = HipRenderer(2, devices=devices)
    try:
        for name in ("gi", "whitted_lds_65", "shard"):
            _, w, h, spp, _ = rv.CASES[name]
            n, nv = 3 * w * h, w * h
            r.spp = spp
            out = torch.empty(pad + n + pad, dtype=torch.float32, device=dev)
            outv = torch.empty(pad + nv + pad, dtype=torch.float32, device=dev)
            # queued on the current stream, not waited for: the render must order itself behind them
            out.fill_(-7.0)
            outv.fill_(-7.0)
            st = r.render_var_device(rv.scene(name), w, h, out.data_ptr() + 4 * pad, outv.data_ptr() + 4 * pad,
                                     after_stream=torch.cuda.current_stream().cuda_stream, **render_kw(name))
            torch.cuda.synchronize()
            got, gotv = out.cpu().numpy(), outv.cpu().numpy()
            assert (got[:pad] == -7.0).all() and (got[pad + n:] == -7.0).all()
            assert (gotv[:pad] == -7.0).all() and (gotv[pad + nv:] == -7.0).all()
            frame = got[pad:pad + n].reshape(h, w, 3)
            assert_frame(frame, rv.oracle_frame(name)[0])
            assert_same_bits(gotv[pad:pad + nv].reshape(h, w), rv.reference(name)[1], name)
            assert st.path_slots == len(rv.shard_pixels(w, h, **{k: v for k, v in rv.CASES[name][4].items() if k.startswith("shard")}))
            # xrt_tonemap and xrt_denoise with a NULL colour read this frame
            assert np.array_equal(r.tonemap(w, h, 1.2), pyoracle.tonemap(frame, 1.2))
            assert_same_bits(r.denoise(None, {}, iterations=2, width=w, height=h), dr.denoise(frame, {}, iterations=2))
    finally:
        r.close()


def test_host_entry_point_on_two_devices():
    r = HipRenderer(2, devices=[0, 0])
    try:
        for name in ("direct", "whitted_bvh_2"):
            _, w, h, _, _ = rv.CASES[name]
            img, var, st = check_case(r, name, abi.XRT_SCHED_WHITTED_BVH if name in rv.WHITTED_BVH else abi.XRT_SCHED_WAVEFRONT)
            assert st.path_slots == w * h
            assert np.array_equal(r.tonemap(w, h, 1.2), pyoracle.tonemap(img, 1.2))
    finally:
        r.close()


# 7. the schedule flags and the launch geometry change nothing; XRT_FLAG_TIMING fills kernel_ms
@pytest.mark.parametrize("kw", [dict(schedule="step"), dict(schedule="step_tri"), dict(schedule="wavefront"),
                                dict(slots_per_wave=16, visits_per_launch=3), dict(visits_per_launch=128),
                                dict(group=False, spec=False, deep="single")])
def test_flags_change_nothing(hr, kw):
    _, _, plain = check_case(hr, "gi")
    _, _, st = check_case(hr, "gi", **kw)
    assert stable(st) == stable(plain)
    _, _, st = check_case(hr, "direct", **kw)
    assert st.schedule == abi.XRT_SCHED_WAVEFRONT


def test_timing_flag(hr):
    _, _, st = check_case(hr, "gi", timing=True)
    for k in (abi.XRT_K_SEED, abi.XRT_K_SHADE, abi.XRT_K_TRACE, abi.XRT_K_FINISH):
        assert st.kernel_ms[k] > 0, k
    _, _, st = check_case(hr, "whitted_lds_2", abi.XRT_SCHED_WHITTED, timing=True)
    assert st.kernel_ms[abi.XRT_K_STEP] > 0 and st.kernel_ms[abi.XRT_K_FINISH] > 0
    _, _, st = check_case(hr, "gi")
    assert sum(st.kernel_ms) == 0


# 8. refusals
def test_refusals():
    hr = HipRenderer(2)   # a context that no medium was ever set on
    try:
        refusals(hr)
    finally:
        hr.close()


def refusals(hr):
    lib = abi.lib()
    s = scenes.cornell(8, 6)
    hr.spp = 2
    hr._uploaded = None
    hr.upload(s)
    img, var = np.zeros((6, 8, 3), np.float32), np.zeros((6, 8), np.float32)

    def rc(p, ctx=hr.ctx, rgb=img, v=var):
        return lib.xrt_render_var(ctx, C.byref(p) if p is not None else None, abi.fptr(rgb) if rgb is not None else None,
                                  abi.fptr(v) if v is not None else None, None)

    ok = hr.params(s, 8, 6)
    assert rc(ok) == 0
    assert rc(ok, ctx=None) == abi.XRT_ERR_INVALID
    assert rc(None) == abi.XRT_ERR_INVALID
    assert rc(ok, rgb=None) == abi.XRT_ERR_INVALID
    assert rc(ok, v=None) == abi.XRT_ERR_INVALID
    assert lib.xrt_render_var_device(hr.ctx, C.byref(ok), None, None, None, None) == abi.XRT_ERR_INVALID
    for spp in (0, 1):
        hr.spp = spp
        assert rc(hr.params(s, 8, 6)) == abi.XRT_ERR_INVALID
        assert b"spp" in lib.xrt_last_error(hr.ctx)
    hr.spp = 2
    assert rc(hr.params(s, 8, 6, accumulate=True)) == abi.XRT_ERR_UNSUPPORTED
    # what xrt_render refuses, the same way
    assert rc(hr.params(s, 8, 6, slots_per_wave=5)) == abi.XRT_ERR_INVALID
    assert rc(hr.params(s, 8, 6, shard_index=2, shard_count=2)) == abi.XRT_ERR_INVALID
    assert rc(hr.params(s, 8, 6, integrator="vpt")) == abi.XRT_ERR_STATE     # no medium
    glass = rv.scene("whitted_lds_2")
    hr._uploaded = None
    hr.upload(glass)
    img, var = np.zeros((12, 16, 3), np.float32), np.zeros((12, 16), np.float32)
    assert rc(hr.params(glass, 16, 12, integrator="gi"), rgb=img, v=var) == abi.XRT_ERR_UNSUPPORTED   # glass outside Whitted
    assert rc(hr.params(glass, 16, 12, integrator="whitted", max_depth=abi.XRT_WHITTED_MAX_DEPTH + 1), rgb=img,
              v=var) == abi.XRT_ERR_UNSUPPORTED
    mesh = rv.scene("whitted_bvh_2")
    hr._uploaded = None
    hr.upload(mesh)
    assert rc(hr.params(mesh, 16, 12, integrator="whitted", max_depth=3), rgb=img, v=var) == abi.XRT_ERR_UNSUPPORTED   # no flag
    assert rc(hr.params(mesh, 16, 12, integrator="whitted", max_depth=3, whitted_bvh=True), rgb=img, v=var) == 0
    hr._uploaded = None


# 9. the chain on the device: render_var_device -> render_aov_device -> denoise_var_device with that
#    variance, against the restatement of the filter applied to those GPU outputs
def test_chain_on_the_device():
    import torch

    w, h, spp = 64, 48, 16
    s = scenes.cornell(w, h)
    r = HipRenderer(spp)
    try:
        f32 = dict(dtype=torch.float32, device="cuda:0")
        frame, var = torch.empty(h, w, 3, **f32), torch.empty(h, w, **f32)
        g = dict(albedo=torch.empty(h, w, 3, **f32), normal=torch.empty(h, w, 3, **f32), depth=torch.empty(h, w, **f32),
                 object=torch.empty(h, w, dtype=torch.int32, device="cuda:0"))
        out, outv = torch.empty(h, w, 3, **f32), torch.empty(h, w, **f32)
        stream = torch.cuda.current_stream().cuda_stream
        r.render_var_device(s, w, h, frame.data_ptr(), var.data_ptr(), after_stream=stream, integrator="gi")
        r.render_aov_device(s, w, h, {k: v.data_ptr() for k, v in g.items()}, after_stream=stream)
        kw = dict(iterations=4, sigma_luminance=4.0, sigma_normal=0.5, sigma_depth=32.0, sigma_albedo=0.2, variance_radius=3)
        r.denoise_var_device(frame.data_ptr(), {k: v.data_ptr() for k, v in g.items()}, out.data_ptr(), w, h,
                             variance_ptr=var.data_ptr(), out_variance_ptr=outv.data_ptr(), after_stream=stream, **kw)
        torch.cuda.synchronize()
        frame, var, out, outv = (t.cpu().numpy() for t in (frame, var, out, outv))
        g = {k: v.cpu().numpy() for k, v in g.items()}
    finally:
        r.close()
    assert (var > 0).sum() > 1000 and (var == 0).sum() > 1000
    ref, ref_var = dv.denoise_var(frame, g, var, **kw)
    assert_same_bits(out, ref)
    assert_same_bits(outv, ref_var)
    est, _ = dv.denoise_var(frame, g, None, **kw)
    assert not np.array_equal(ref.view(np.uint32), est.view(np.uint32))   # the plane was read, not the estimate


# 10. examples/render_var.cpp through the C++ API (HipRenderer::renderVariance, denoiseVar with a variance)
def test_render_var_example_ppm(tmp_path):
    w, h, spp = 48, 36, 4
    prefix = tmp_path / "frame"
    run_example("render_var", w, h, spp, prefix)
    # examples/denoise.cpp's scene: the example's plane and sphere under a QuadLight, GIIntegrator(3)
    s = scenes.SceneBundle()
    s.add_mesh("plane", scenes.EXAMPLE_PLANE, (1.0, 1.0, 1.0))
    s.add_sphere("sphere_diffuse", (0.0, 0.0, 0.0), 1.0, (0.58, 0.58, 0.58))
    s.add_quad_light("QuadLight", (1.0, 4.0, -1.0), (1.0, 4.0, 1.0), (-1.0, 4.0, -1.0), (25.0, 25.0, 25.0))
    s.flatten()
    s.camera = scenes.pinhole((1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 8, 1), 60.0, w, h)
    s.integrator, s.max_depth = "gi", 3
    frame, var, _ = rv.render(s, w, h, spp)
    assert np.array_equal(frame.view(np.uint32), pyoracle.render(s, w, h, spp)[0].view(np.uint32))
    planes, _, _ = ar.render(s, w, h, spp)
    assert frame.max() > 0 and (var > 0).any()
    assert np.array_equal(read_ppm(tmp_path / "frame.noisy.ppm", w, h), pyoracle.tonemap(frame, 1.2).astype(np.int64))
    want, _ = dv.denoise_var(frame, planes, var, **dv.DEFAULTS)
    assert np.array_equal(read_ppm(tmp_path / "frame.denoised.ppm", w, h), pyoracle.tonemap(want, 1.2).astype(np.int64))
