"""XRT_INTEGRATOR_WHITTED over triangle scenes beyond LDS (XRT_FLAG_WHITTED_BVH, k_whitted_bvh
in whitted.hip) against the restatement (tests/whitted_restatement.py, a linear scan over every
triangle): every frame bit for bit, every counter for equality, the schedule
XRT_SCHED_WHITTED_BVH.  The scenes and the conditions they are chosen for are in
tests/whitted_bvh_scenes.py and checked without a GPU in tests/test_whitted_bvh_restatement.py."""
import numpy as np
import pytest

import pyoracle
import whitted_bvh_scenes as wb
import whitted_scenes as ws
from gpu_checks import DATA_DIR, assert_frame, assert_same_bits, check_whitted_case, read_ppm, render_rc, run_example
from xraytracer_amd import abi
from xraytracer_amd.renderer import HipRenderer

pytestmark = pytest.mark.gpu


def check_case(name, devices=None):
    """render wb.CASES[name] on the GPU with the flag and compare frame, counters and schedule
    with the restatement"""
    return check_whitted_case(wb, name, abi.XRT_SCHED_WHITTED_BVH, devices=devices, whitted_bvh=True)


# 1. two-level, glass: the small objects' LDS scan merged with the mesh's BVH walk
def test_two_level_glass():
    _, cnt, per = check_case("glass")
    assert cnt["whit_refract"] > 0 and cnt["whit_depth_cut"] > 0
    assert 0 < per["shadow_hit"].sum() < cnt["shadow_rays"]


def test_pinned_two_level_scene_renders_with_the_flag():
    check_case("pinned")


# 2. two-level, metal: non-unit directions in the BVH walk, chains that end on Lambert walls
def test_two_level_metal():
    _, cnt, per = check_case("metal_9")
    assert ((per["rays"] > 1) & (per["shadow"] > 0)).any()


# 3. / 4. one-level scenes: only large meshes; only medium ones (every triangle in the BVH)
def test_one_level_big_meshes():
    _, cnt, _ = check_case("big_meshes")
    assert cnt["whit_refract"] > 0 and cnt["whit_tir"] > 0


def test_one_level_medium_meshes():
    _, cnt, per = check_case("medium_meshes")
    assert 0 < per["shadow_hit"].sum() < cnt["shadow_rays"]


# 5. ties across the two levels: the restatement decides which of two coincident triangles wins
@pytest.mark.parametrize("name", ["tie_before", "tie_after"])
def test_ties_across_the_levels(name):
    check_case(name)
    assert wb.reference("tie_before")[1]["whit_rays"] != wb.reference("tie_after")[1]["whit_rays"]


# 6. ties inside the BVH: two coincident meshes, every hit resolves to the first
def test_ties_inside_the_bvh():
    _, cnt, _ = check_case("twins")
    assert cnt["whit_rays"] == cnt["samples"]


# 7. the quad emitter: shadow rays cross it unoccluded, camera hits on it add nothing
def test_emitter():
    _, _, per = check_case("emitter")
    s = wb.scene("emitter")
    emitters = [i for i in range(s.desc.n_objects) if s.desc.objects[i].light >= 0]
    on_emitter = np.isin(per["first_obj"], emitters)
    assert on_emitter.any() and not per["radiance"][on_emitter].any()


# 8. plumbing: a shard, accumulation, a window crossing, a multi-device context
@pytest.mark.parametrize("name", ["glass_shard", "glass_accumulate", "glass_70"])
def test_plumbing(name):
    check_case(name)


def test_multi_device_context():
    check_case("glass", devices=[0, 0])


def test_timing_flag():
    _, w, h, spp, depth, _ = wb.CASES["glass"]
    ref, _, _ = wb.reference("glass")
    r = HipRenderer(spp)
    try:
        img = r.render(wb.scene("glass"), w, h, max_depth=depth, whitted_bvh=True, timing=True)
        assert r.stats.schedule == abi.XRT_SCHED_WHITTED_BVH
        assert_frame(img, ref)
        assert r.stats.launches[abi.XRT_K_STEP] == 1 and r.stats.kernel_ms[abi.XRT_K_STEP] > 0.0
    finally:
        r.close()


def test_lds_scene_is_unchanged_by_the_flag():
    """a scene that fits LDS renders through k_whitted with or without the flag: same bits,
    XRT_SCHED_WHITTED"""
    _, w, h, spp, depth, _ = ws.CASES["example"]
    ref, cnt, _ = ws.reference("example")
    r = HipRenderer(spp)
    try:
        plain = r.render(ws.scene("example"), w, h, max_depth=depth)
        assert r.stats.schedule == abi.XRT_SCHED_WHITTED
        flagged = r.render(ws.scene("example"), w, h, max_depth=depth, whitted_bvh=True)
        assert r.stats.schedule == abi.XRT_SCHED_WHITTED
        assert {k: int(getattr(r.stats, k)) for k in ws.COUNTERS} == {k: int(cnt[k]) for k in ws.COUNTERS}
        assert_same_bits(flagged, plain)
        assert_frame(flagged, ref)
    finally:
        r.close()


# 9. refusals
def test_glass_depth_limit_holds_with_the_flag():
    rc, msg = render_rc(wb.scene("glass"), 24, 18, 1, max_depth=abi.XRT_WHITTED_MAX_DEPTH + 1, whitted_bvh=True)
    assert rc == abi.XRT_ERR_UNSUPPORTED and "XRT_WHITTED_MAX_DEPTH" in msg


def test_without_the_flag_the_refusal_is_unchanged():
    rc, msg = render_rc(wb.scene("glass"), 24, 18, 1)
    assert rc == abi.XRT_ERR_UNSUPPORTED and "LDS" in msg and "XRT_FLAG_WHITTED_BVH" not in msg


def test_scene_without_a_triangle_bvh_is_refused():
    s = wb.mixed_beyond_lds(24, 18)
    rc, msg = render_rc(s, 24, 18, 1, whitted_bvh=True)
    assert rc == abi.XRT_ERR_UNSUPPORTED and "triangle BVH" in msg
    rc, msg = render_rc(s, 24, 18, 1)
    assert rc == abi.XRT_ERR_UNSUPPORTED and "LDS" in msg


# 10. examples/whitted_mesh.cpp: scene "glass" through the C++ API, which sets the flag itself
def test_whitted_mesh_example_ppm(tmp_path):
    _, w, h, spp, _, _ = wb.CASES["glass"]
    out = tmp_path / "whitted_mesh.ppm"
    log = run_example("whitted_mesh", w, h, spp, out, env={"XRT_DATA_DIR": DATA_DIR})
    assert f"(schedule {abi.XRT_SCHED_WHITTED_BVH})" in log
    ref, _, _ = wb.reference("glass")
    assert np.array_equal(read_ppm(out, w, h), pyoracle.tonemap(ref, 1.2).astype(np.int64))
