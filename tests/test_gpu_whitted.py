"""XRT_INTEGRATOR_WHITTED on the GPU (whitted.hip) against the restatement
(tests/whitted_restatement.py): every frame bit for bit, every counter for equality.  The
scenes and the conditions they are chosen for are in tests/whitted_scenes.py and checked
without a GPU in tests/test_whitted_restatement.py."""
import json
import os

import numpy as np
import pytest

import pyoracle
import whitted_scenes as ws
from gpu_checks import ROOT, assert_frame, check_whitted_case, read_ppm, render_rc, run_example, words
from xraytracer_amd import abi, scenes
from xraytracer_amd.renderer import HipRenderer

pytestmark = pytest.mark.gpu


def check_case(name, devices=None):
    """render CASES[name] on the GPU and compare frame and counters with the restatement"""
    return check_whitted_case(ws, name, abi.XRT_SCHED_WHITTED, devices=devices)


# 1. Lambert + both light kinds: the example scene, a shard of it, accumulation over an image
@pytest.mark.parametrize("name", ["example", "example_shard", "example_accumulate"])
def test_example_scene(name):
    _, cnt, per = check_case(name)
    assert 0 < per["shadow_hit"].sum() < cnt["shadow_rays"]


# 2. stream crossing: a 64-sample window (spp 70), the 624-word block at sample 312 (spp 330)
@pytest.mark.parametrize("name", ["stream_70", "stream_330"])
def test_stream_crossing(name):
    _, cnt, _ = check_case(name)
    assert cnt["draws"] == 2 * cnt["samples"]
    spp = ws.CASES[name][3]
    assert cnt["rng_twists"] == 48 * ((2 * spp + 623) // 624) and (name != "stream_330" or cnt["rng_twists"] == 96)


# 3. mirror chain: non-unit directions, depth cuts, chains that end on the Lambert floor
@pytest.mark.parametrize("name", ["mirrors_3", "mirrors_9"])
def test_mirror_chain(name):
    _, cnt, per = check_case(name)
    assert cnt["whit_depth_cut"] > 0
    assert ((per["rays"] > 1) & (per["shadow"] > 0)).any()


# 4. glass tree: refraction, total internal reflection, the full tree (the lane ring at its bound)
@pytest.mark.parametrize("name", ["glass_3", "glass_max"])
def test_glass_tree(name):
    _, cnt, per = check_case(name)
    depth = ws.CASES[name][4]
    assert cnt["whit_refract"] > 0 and cnt["whit_tir"] > 0 and cnt["whit_depth_cut"] > 0
    assert (per["cut"] == 2 ** (depth + 1)).any()


def test_glass_depth_limit():
    rc, msg = render_rc(ws.scene("glass_max"), 16, 12, 1, max_depth=abi.XRT_WHITTED_MAX_DEPTH + 1)
    assert rc == abi.XRT_ERR_UNSUPPORTED and "XRT_WHITTED_MAX_DEPTH" in msg


# 5. each scene kind: triangles only, spheres only (scanned, and through the sphere BVH)
@pytest.mark.parametrize("name", ["cornell_tri", "spheres_small", "spheres_bvh"])
def test_scene_kinds(name):
    check_case(name)


# 6. no-material and emitter objects
def test_emitter_and_no_material():
    _, cnt, per = check_case("cornell_emitter")
    s = ws.scene("cornell_emitter")
    emitters = [i for i in range(s.desc.n_objects) if s.desc.objects[i].light >= 0]
    on_emitter = np.isin(per["first_obj"], emitters)
    assert on_emitter.any() and not per["radiance"][on_emitter].any()


def test_medium_box_has_no_material():
    _, _, per = check_case("medium_box")
    s = ws.scene("medium_box")
    boxes = [i for i in range(s.desc.n_objects) if s.desc.objects[i].kind == abi.XRT_OBJ_BOX]
    on_box = np.isin(per["first_obj"], boxes)
    assert on_box.any() and not per["radiance"][on_box].any()


# 7. rejection: a point light with negative intensity
def test_rejection():
    _, cnt, _ = check_case("rejection")
    assert cnt["rejected"] > 0


# 8. edges
def test_max_depth_zero():
    _, cnt, _ = check_case("mirrors_0")
    assert cnt["whit_depth_cut"] > 0


def test_zero_delta_lights():
    _, cnt, _ = check_case("no_lights")
    assert cnt["shadow_rays"] == 0


def test_clearing_delta_lights():
    """xrt_set_delta_lights(n = 0) after a non-empty set: the lights are gone, the scene stays"""
    _, w, h, spp, depth, _ = ws.CASES["no_lights"]
    ref, cnt, _ = ws.reference("no_lights")
    lit = ws.example(w, h)
    r = HipRenderer(spp)
    try:
        with_lights = r.render(lit, w, h, max_depth=depth)
        assert r.stats.shadow_rays > 0
        assert abi.lib().xrt_set_delta_lights(r.ctx, None, 0) == 0
        img = r.render(lit, w, h, max_depth=depth)   # same bundle: no re-upload
        assert r.stats.shadow_rays == 0
        assert_frame(img, ref)
        assert not np.array_equal(words(img), words(with_lights))
    finally:
        r.close()


def test_mirror_materials_need_whitted():
    rc, msg = render_rc(ws.scene("mirrors_3"), 24, 18, 1, integrator="gi")
    assert rc == abi.XRT_ERR_UNSUPPORTED and "Whitted" in msg
    rc, msg = render_rc(ws.scene("glass_3"), 16, 12, 1, integrator="normal")
    assert rc == abi.XRT_ERR_UNSUPPORTED


def test_two_level_scene_is_unsupported():
    s = scenes.cornell_spheremesh(24, 18, n_theta=40, n_phi=40)
    s.add_point_light("PointLight", ws.translate(278.0, 400.0, 279.5), (1.0, 1.0, 1.0), 1.0e5)
    rc, msg = render_rc(s, 24, 18, 1, integrator="whitted")
    assert rc == abi.XRT_ERR_UNSUPPORTED and "LDS" in msg


# 9. multi-device context over one GPU listed twice
def test_multi_device_context():
    check_case("example", devices=[0, 0])
    check_case("glass_3", devices=[0, 0])


# 10. the kernel's reflect / refract / fresnel / normalize against the reference's geometry.cpp
def test_device_whitted_math(gpu):
    with open(os.path.join(ROOT, "tests", "golden", "ref_whitted_kats.json")) as f:
        g = json.load(f)
    vin = np.ascontiguousarray(np.array(g["math"]["in"], np.uint32).view(np.float32))
    want = np.array(g["math"]["out"], np.uint32)
    out = np.zeros((len(vin), 13), np.float32)
    assert abi.lib().xrt_test_whitted_math(gpu, abi.fptr(vin), len(vin), abi.fptr(out)) == 0
    got = out.view(np.uint32)
    bad = np.argwhere(got != want)
    both_nan = np.isnan(out) & np.isnan(want.view(np.float32))
    print(f"whitted math: {len(bad)} of {got.size} words differ, {int((both_nan & (got != want)).sum())} of them NaN on both sides")
    assert len(bad) == 0, [(int(i), int(j), hex(got[i, j]), hex(want[i, j])) for i, j in bad[:5]]


# 11. examples/whitted.cpp through the C++ API
def test_whitted_example_ppm(tmp_path):
    w, h, spp = 48, 36, 3
    out = tmp_path / "whitted.ppm"
    run_example("whitted", w, h, spp, out)
    ref, _, _ = ws.reference("example")
    assert np.array_equal(read_ppm(out, w, h), pyoracle.tonemap(ref, 1.2).astype(np.int64))
