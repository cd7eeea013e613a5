"""xrt_render_var under XRT_FLAG_VAR_FUSED on the GPU (the moments builds of k_step, k_step_tri and
k_step_merged) against the restatement (tests/render_var_restatement.py): the frame bit for bit the
oracle's, the variance plane bit for bit the restatement's, the schedule the fused or merged one
the case names, and the counters those of xrt_render for the same keywords with spec=False and
schedule="step".  The cases are in tests/render_var_fused_cases.py and checked without a GPU in
tests/test_render_var_fused_cases.py.  Without the feature the flag changes nothing and every
schedule below is XRT_SCHED_WAVEFRONT."""
import ctypes as C
import os

import numpy as np
import pytest

import camlist_restatement as cr
import denoise_var_restatement as dv
import pyoracle
import render_var_fused_cases as fc
import render_var_restatement as rv
import whitted_scenes as ws
from gpu_checks import assert_frame, assert_same_bits, counters_equal, read_ppm, run_example, words
from test_gpu_render_var import stable   # over its STABLE counter set
from xraytracer_amd import abi, scenes
from xraytracer_amd.renderer import HipRenderer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hr():
    r = HipRenderer(2, device=0)
    yield r
    r.close()


def check(hr, scene, w, h, spp, sem, geo, sched, reference, oracle):
    """one fused variance render: frame, plane, schedule, the oracle's counters, and xrt_render's stats
    for the same keywords with spec=False and schedule="step"; returns (frame, plane, stats)"""
    hr.spp = spp
    hr._uploaded = None
    img, var = hr.render_var(scene, w, h, fused_var=True, **sem, **geo)
    st = hr.stats
    print(f"schedule {st.schedule} slots_per_wave {st.slots_per_wave} group_lanes {st.group_lanes} iterations {st.iterations} "
          f"step launches {st.launches[abi.XRT_K_STEP]} twists {st.rng_twists} rejected {st.rejected}")
    assert st.schedule == sched
    assert_frame(img, oracle[0])
    assert_same_bits(var, reference[1])
    counters_equal(st, oracle[1])
    kw = dict(geo)
    kw.setdefault("schedule", "step")
    assert_frame(hr.render(scene, w, h, spec=False, **sem, **kw), img)
    assert stable(hr.stats) == stable(st)
    return img, var, st


def check_case(hr, name):
    scene_name, w, h, spp, sem, geo, sched = fc.CASES[name]
    return check(hr, fc.scene(scene_name), w, h, spp, sem, geo, sched, fc.reference(name), fc.oracle_frame(name))


# 1. the merged kernel: every layout, both integrators, launch boundaries, two lights, rejects
@pytest.mark.parametrize("name", sorted(n for n in fc.CASES if n.startswith(("merged_", "two_lights_"))))
def test_merged_layouts(hr, name):
    _, _, st = check_case(hr, name)
    geo = fc.CASES[name][5]
    if "visits_per_launch" in geo:
        assert st.visits_per_launch == geo["visits_per_launch"] and st.iterations > 5


@pytest.mark.parametrize("name", ["rejects_gi", "rejects_direct"])
def test_rejects(hr, name):
    _, _, st = check_case(hr, name)
    assert st.rejected > 1000


def test_in_launch_twists(hr):
    _, _, st = check_case(hr, "twists")
    assert st.rng_twists > st.path_slots


# 2. the pixels k_camlist retires never reach a step kernel: their records are +0 whatever an earlier render left
def test_retired_pixels_after_a_direct_render(hr):
    check_case(hr, "merged_direct_64_pairs")   # Direct's misses add 0.18 per sample: non-zero records for the empty pixels
    _, var, _ = check_case(hr, "merged_gi_64_pairs")
    empty = cr.empty_pixels(fc.scene("cornell_64"), 64, 48)
    assert empty.sum() >= 100 and not words(var)[empty].any()


# 3. partition groups on streams of their own, one launch per round, the interleaved slot map
def test_partition_groups_and_interleave(hr):
    _, _, g = check_case(hr, "groups_256")
    assert g.partitions == 16 and g.launches[abi.XRT_K_STEP] > g.iterations
    _, _, f = check_case(hr, "no_overlap_256")
    assert f.launches[abi.XRT_K_STEP] == f.iterations
    _, _, i = check_case(hr, "interleave_256")
    assert i.launches[abi.XRT_K_STEP] > i.iterations
    scene_name, w, h, _, sem, geo, _ = fc.CASES["interleave_256"]
    m = hr.slot_map(fc.scene(scene_name), w, h, **sem, **geo)
    assert not np.array_equal(m, np.arange(w * h))   # a variance render through a map that is not the identity


# 4. the two-level form, k_step_tri, k_step
@pytest.mark.parametrize("name", sorted(n for n in fc.CASES if n.startswith(("two_level_", "step_tri_", "kstep_"))))
def test_two_level_step_tri_and_kstep(hr, name):
    check_case(hr, name)


@pytest.mark.parametrize("name", fc.KSTEP_FROM_RV)
def test_kstep_over_the_wavefront_cases(hr, name):
    _, w, h, spp, sem = rv.CASES[name]
    check(hr, rv.scene(name), w, h, spp, sem, {}, abi.XRT_SCHED_STEP, rv.reference(name), rv.oracle_frame(name))


# 5. where the flag changes nothing
def test_wavefront_and_whitted_fall_through(hr):
    for name, kw, sched in (("gi", dict(schedule="wavefront"), abi.XRT_SCHED_WAVEFRONT),
                            ("whitted_lds_65", {}, abi.XRT_SCHED_WHITTED)):
        _, w, h, spp, sem = rv.CASES[name]
        hr.spp = spp
        hr._uploaded = None
        img, var = hr.render_var(rv.scene(name), w, h, fused_var=True, **sem, **kw)
        st = hr.stats
        assert st.schedule == sched
        assert_frame(img, rv.oracle_frame(name)[0])
        assert_same_bits(var, rv.reference(name)[1], name)
        img0, var0 = hr.render_var(rv.scene(name), w, h, **sem, **kw)
        assert_same_bits(img0, img)
        assert_same_bits(var0, var)
        assert stable(hr.stats) == stable(st)
        if name.startswith("whitted"):
            cnt = rv.oracle_frame(name)[1]
            assert {k: int(getattr(st, k)) for k in ws.COUNTERS} == {k: int(cnt[k]) for k in ws.COUNTERS}


def test_render_ignores_the_flag(hr):
    for name in ("merged_gi_64_pairs", "merged_direct_64_pairs"):
        scene_name, w, h, spp, sem, _, _ = fc.CASES[name]
        hr.spp = spp
        hr._uploaded = None
        plain = hr.render(fc.scene(scene_name), w, h, **sem)
        st = stable(hr.stats)
        assert_same_bits(hr.render(fc.scene(scene_name), w, h, fused_var=True, **sem), plain)
        assert stable(hr.stats) == st
        assert_frame(plain, fc.oracle_frame(name)[0])


def test_refusals_stay():
    hr = HipRenderer(2)
    try:
        lib = abi.lib()
        s = scenes.cornell(8, 6)
        hr.upload(s)
        img, var = np.zeros((6, 8, 3), np.float32), np.zeros((6, 8), np.float32)

        def rc(p):
            return lib.xrt_render_var(hr.ctx, C.byref(p), abi.fptr(img), abi.fptr(var), None)

        assert rc(hr.params(s, 8, 6, fused_var=True)) == 0
        assert rc(hr.params(s, 8, 6, fused_var=True, accumulate=True)) == abi.XRT_ERR_UNSUPPORTED
        assert rc(hr.params(s, 8, 6, fused_var=True, slots_per_wave=5)) == abi.XRT_ERR_INVALID
        for spp in (0, 1):
            hr.spp = spp
            assert rc(hr.params(s, 8, 6, fused_var=True)) == abi.XRT_ERR_INVALID
            assert b"spp" in lib.xrt_last_error(hr.ctx)
    finally:
        hr.close()


# 6. shards, the device entry point, two devices, the chain into the variance-guided filter
def test_shard_leaves_other_rows_zero(hr):
    _, w, h, spp, sem = rv.CASES["shard"]
    img, var, st = check(hr, rv.scene("shard"), w, h, spp, sem, {}, abi.XRT_SCHED_STEP_MERGED, rv.reference("shard"),
                         rv.oracle_frame("shard"))
    rows = np.arange(12) % 3 == 1
    assert not words(img)[~rows].any() and not words(var)[~rows].any()
    assert (var[rows] > 0).any() and st.samples == 4 * 16 * 4


@pytest.fixture(scope="module")
def chain_reference():
    w, h, spp = 64, 48, 16
    s = scenes.cornell(w, h)
    frame, var, _ = rv.render(s, w, h, spp, integrator="gi")
    return s, frame, var


@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_device_entry_point_and_chain(devices, chain_reference):
    import torch

    w, h, spp, pad = 64, 48, 16, 64
    s, ref_frame, ref_var = chain_reference
    n, nv = 3 * w * h, w * h
    r = HipRenderer(spp, devices=devices)
    try:
        f32 = dict(dtype=torch.float32, device="cuda:0")
        out, outv = torch.empty(pad + n + pad, **f32), torch.empty(pad + nv + pad, **f32)
        out.fill_(-7.0)   # queued on the current stream, not waited for
        outv.fill_(-7.0)
        g = dict(albedo=torch.empty(h, w, 3, **f32), normal=torch.empty(h, w, 3, **f32), depth=torch.empty(h, w, **f32),
                 object=torch.empty(h, w, dtype=torch.int32, device="cuda:0"))
        clean, cleanv = torch.empty(h, w, 3, **f32), torch.empty(h, w, **f32)
        stream = torch.cuda.current_stream().cuda_stream
        st = r.render_var_device(s, w, h, out.data_ptr() + 4 * pad, outv.data_ptr() + 4 * pad, after_stream=stream,
                                 integrator="gi", fused_var=True)
        assert st.schedule == abi.XRT_SCHED_STEP_MERGED and st.path_slots == w * h
        r.render_aov_device(s, w, h, {k: v.data_ptr() for k, v in g.items()}, after_stream=stream)
        kw = dict(iterations=4, sigma_luminance=4.0, sigma_normal=0.5, sigma_depth=32.0, sigma_albedo=0.2, variance_radius=3)
        r.denoise_var_device(out.data_ptr() + 4 * pad, {k: v.data_ptr() for k, v in g.items()}, clean.data_ptr(), w, h,
                             variance_ptr=outv.data_ptr() + 4 * pad, out_variance_ptr=cleanv.data_ptr(), after_stream=stream, **kw)
        torch.cuda.synchronize()
        got, gotv, clean, cleanv = (t.cpu().numpy() for t in (out, outv, clean, cleanv))
        g = {k: v.cpu().numpy() for k, v in g.items()}
    finally:
        r.close()
    assert (got[:pad] == -7.0).all() and (got[pad + n:] == -7.0).all()
    assert (gotv[:pad] == -7.0).all() and (gotv[pad + nv:] == -7.0).all()
    frame, var = got[pad:pad + n].reshape(h, w, 3), gotv[pad:pad + nv].reshape(h, w)
    assert_frame(frame, ref_frame)
    assert_same_bits(var, ref_var)
    want, want_var = dv.denoise_var(ref_frame, g, ref_var, **kw)   # the restatement's chain over the device's guide planes
    assert_same_bits(clean, want)
    assert_same_bits(cleanv, want_var)


def test_host_entry_point_on_two_devices():
    r = HipRenderer(2, devices=[0, 0])
    try:
        for name in ("merged_direct_16_group", "step_tri_gi"):
            scene_name, w, h, spp, sem, geo, sched = fc.CASES[name]
            r.spp = spp
            img, var = r.render_var(fc.scene(scene_name), w, h, fused_var=True, **sem, **geo)
            assert r.stats.schedule == sched and r.stats.path_slots == w * h
            assert_frame(img, fc.oracle_frame(name)[0])
            assert_same_bits(var, fc.reference(name)[1])
            counters_equal(r.stats, fc.oracle_frame(name)[1])
    finally:
        r.close()


# 7. HipRenderer::renderVariance's last argument through examples/render_var.cpp
def test_render_variance_fused_in_cpp(hr, tmp_path):
    w, h, spp = 48, 36, 4
    prefix = tmp_path / "frame"
    out = run_example("render_var", w, h, spp, prefix, "fused")
    assert f"schedule {abi.XRT_SCHED_STEP}\n" in out
    # examples/denoise.cpp's scene: the example's plane and sphere under a QuadLight, GIIntegrator(3)
    s = scenes.SceneBundle()
    s.add_mesh("plane", scenes.EXAMPLE_PLANE, (1.0, 1.0, 1.0))
    s.add_sphere("sphere_diffuse", (0.0, 0.0, 0.0), 1.0, (0.58, 0.58, 0.58))
    s.add_quad_light("QuadLight", (1.0, 4.0, -1.0), (1.0, 4.0, 1.0), (-1.0, 4.0, -1.0), (25.0, 25.0, 25.0))
    s.flatten()
    s.camera = scenes.pinhole((1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 8, 1), 60.0, w, h)
    s.integrator, s.max_depth = "gi", 3
    hr.spp = spp
    hr._uploaded = None
    img, var = hr.render_var(s, w, h, fused_var=True)
    assert hr.stats.schedule == abi.XRT_SCHED_STEP
    frame = np.fromfile(os.fspath(prefix) + ".frame.raw", np.float32).reshape(h, w, 3)
    plane = np.fromfile(os.fspath(prefix) + ".variance.raw", np.float32).reshape(h, w)
    assert_same_bits(frame, img)
    assert_same_bits(plane, var)
    ref, ref_var, _ = rv.render(s, w, h, spp)
    assert_frame(img, ref)
    assert_same_bits(var, ref_var)
    assert np.array_equal(read_ppm(tmp_path / "frame.noisy.ppm", w, h), pyoracle.tonemap(ref, 1.2).astype(np.int64))
