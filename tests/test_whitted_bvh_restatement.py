"""The Whitted BVH scenes without a GPU: the restatement alone (a linear scan over every
triangle, tests/whitted_restatement.py) meets each condition the GPU test of that scene relies
on (tests/test_gpu_whitted_bvh.py), the scenes have the sizes that send them down the path they
are named for, and — as tests/test_whitted_restatement.py does for the LDS scenes — the
level-by-level walk equals a scalar FIFO walk for one glass and one metal sample through the
mesh."""
import numpy as np
import pytest

import whitted_bvh_scenes as wb
import whitted_restatement as wr
import whitted_scenes as ws
from test_whitted_restatement import bits, scalar_walk
from xraytracer_amd import abi, renderer

K_SMALL_TRIS, K_LARGE_OBJ_TRIS = 1024, 256   # csrc/wavefront.h kSmallTris, kLargeObjTris


def counts(s):
    return [s.desc.objects[i].count for i in range(s.desc.n_objects)]


def test_flag_and_schedule_constants():
    assert abi.XRT_FLAG_WHITTED_BVH == 512 and abi.XRT_SCHED_WHITTED_BVH == 7
    flags = [abi.XRT_FLAG_TIMING, abi.XRT_FLAG_WAVEFRONT, abi.XRT_FLAG_NO_MERGED, abi.XRT_FLAG_NO_GROUP,
             abi.XRT_FLAG_ACCUMULATE, abi.XRT_FLAG_DEEP_SINGLE, abi.XRT_FLAG_DEEP_QUAD, abi.XRT_FLAG_NO_PIXEL,
             abi.XRT_FLAG_NO_SPEC, abi.XRT_FLAG_WHITTED_BVH]
    assert len(set(flags)) == len(flags) and all(f & (f - 1) == 0 for f in flags)


def test_params_keyword_sets_the_flag():
    s = ws.scene("example")
    r = renderer.HipRenderer.__new__(renderer.HipRenderer)   # params() needs no context
    r.spp = 1
    assert r.params(s, 8, 6).flags & abi.XRT_FLAG_WHITTED_BVH == 0
    assert r.params(s, 8, 6, whitted_bvh=True).flags & abi.XRT_FLAG_WHITTED_BVH
    assert r.params(s, 8, 6, whitted_bvh=True, accumulate=True).flags == abi.XRT_FLAG_WHITTED_BVH | abi.XRT_FLAG_ACCUMULATE
    r.ctx = None


# ---- which path each scene takes (xrt_upload_scene's split, by the sizes alone) ----
@pytest.mark.parametrize("name", ["glass", "metal_9", "pinned", "tie_before", "tie_after", "twins", "emitter"])
def test_two_level_scenes(name):
    c = counts(wb.scene(name))
    small = [n for n in c if n <= K_LARGE_OBJ_TRIS]
    assert sum(c) > K_SMALL_TRIS and any(n > K_LARGE_OBJ_TRIS for n in c) and small and sum(small) <= K_SMALL_TRIS


def test_one_level_scenes():
    big = counts(wb.scene("big_meshes"))
    assert len(big) == 2 and min(big) > K_LARGE_OBJ_TRIS   # no small object: no two-level split
    med = counts(wb.scene("medium_meshes"))
    assert len(med) >= 7 and max(med) <= K_LARGE_OBJ_TRIS and sum(med) > K_SMALL_TRIS   # no large object


def test_mixed_scene_exceeds_the_lds_carve():
    d = wb.mixed_beyond_lds(8, 6).desc
    assert d.n_spheres == 1 and d.n_tris * 112 > 64 * 1024   # step_layout: 48 + 16 + 48 bytes per triangle


# ---- scene coverage: the restatement alone meets the conditions the GPU tests state ----
def test_cover_two_level_glass():
    for name in ("glass", "emitter", "glass_shard", "glass_accumulate", "glass_70"):
        _, cnt, per = wb.reference(name)
        assert cnt["whit_refract"] > 0 and cnt["whit_depth_cut"] > 0
        assert 0 < per["shadow_hit"].sum() < cnt["shadow_rays"]
        assert ((per["shadow"] > 0) & (per["shadow_hit"] == 0)).any()   # lit samples
    s = wb.scene("glass")
    assert s.desc.objects[wb.object_index(s, wb.MESH)].material == abi.XRT_MAT_GLASS
    assert (ws_first(wb.reference("glass")) == wb.object_index(s, wb.MESH)).any()
    full, shard, acc = (wb.reference(n)[0] for n in ("glass", "glass_shard", "glass_accumulate"))
    assert np.array_equal(shard[1::3], full[1::3]) and not shard[0::3].any() and not shard[2::3].any()
    assert not np.array_equal(acc, full)
    assert wb.reference("glass_70")[1]["draws"] == 2 * 48 * 70   # crosses the 64-sample window


def ws_first(ref):
    return ref[2]["first_obj"]


def test_cover_pinned_scene():
    s = wb.scene("pinned")
    assert s.desc.objects[wb.object_index(s, wb.MESH)].count == 3200
    _, cnt, per = wb.reference("pinned")
    assert (ws_first(wb.reference("pinned")) == wb.object_index(s, wb.MESH)).any()
    assert 0 < per["shadow_hit"].sum() < cnt["shadow_rays"]


def test_cover_two_level_metal():
    s = wb.scene("metal_9")
    _, cnt, per = wb.reference("metal_9")
    on_mesh = ws_first(wb.reference("metal_9")) == wb.object_index(s, wb.MESH)
    assert on_mesh.any() and (per["rays"][on_mesh] > 1).all()         # a non-unit child through the scene
    assert ((per["rays"] > 1) & (per["shadow"] > 0)).any()            # chains that end on a Lambert wall
    assert cnt["whit_refract"] == 0 and cnt["whit_tir"] == 0


def test_cover_one_level_big_meshes():
    s = wb.scene("big_meshes")
    _, cnt, per = wb.reference("big_meshes")
    assert cnt["whit_refract"] > 0 and cnt["whit_tir"] > 0 and cnt["whit_depth_cut"] > 0
    first = ws_first(wb.reference("big_meshes"))
    assert (first == wb.object_index(s, "ground")).any() and (first == wb.object_index(s, "ball")).any() and (first < 0).any()
    assert 0 < per["shadow_hit"].sum() < cnt["shadow_rays"]
    assert wr.delta_lights(s)[0][0] == abi.XRT_DLIGHT_DISTANT and len(wr.delta_lights(s)) == 1


def test_cover_one_level_medium_meshes():
    s = wb.scene("medium_meshes")
    _, cnt, per = wb.reference("medium_meshes")
    assert 0 < per["shadow_hit"].sum() < cnt["shadow_rays"]   # shadow rays both hit and missed
    mats = {s.desc.objects[i].material for i in range(s.desc.n_objects)}
    assert {abi.XRT_MAT_LAMBERT, abi.XRT_MAT_METAL, abi.XRT_MAT_GLASS} <= mats
    assert cnt["whit_refract"] > 0 and cnt["whit_depth_cut"] > 0 and (per["rays"] > 1).any()


def test_cover_ties_across_the_levels():
    sb, sa = wb.scene("tie_before"), wb.scene("tie_after")
    ib, ia = wb.object_index(sb, sb.tie_name), wb.object_index(sa, sa.tie_name)
    assert ib < wb.object_index(sb, wb.MESH) and ia > wb.object_index(sa, wb.MESH)
    # the copy's vertices are bitwise those of a mesh triangle
    for s, i in ((sb, ib), (sa, ia)):
        m = s.desc.objects[wb.object_index(s, wb.MESH)]
        mesh = s.triangles()[m.first:m.first + m.count].view(np.uint32).reshape(-1, 9)
        copy = s.triangles()[s.desc.objects[i].first].view(np.uint32).reshape(9)
        assert (mesh == copy).all(axis=1).sum() == 1
        assert s.desc.objects[i].material == abi.XRT_MAT_LAMBERT and m.material == abi.XRT_MAT_METAL
    (_, cb, pb), (_, ca, pa) = wb.reference("tie_before"), wb.reference("tie_after")
    hit = pb["first_obj"] == ib
    assert hit.any()                               # some samples do hit that triangle: the copy wins before,
    assert (pa["first_obj"][hit] == wb.object_index(sa, wb.MESH)).all() and not (pa["first_obj"] == ia).any()   # the mesh after
    assert (pb["rays"][hit] == 1).all() and (pa["rays"][hit] > 1).all()
    assert cb["whit_rays"] != ca["whit_rays"]


def test_cover_ties_inside_the_bvh():
    s = wb.scene("twins")
    first, second = (wb.object_index(s, n) for n in s.twin_order)
    assert first < second
    assert s.desc.objects[first].material == abi.XRT_MAT_LAMBERT and s.desc.objects[second].material == abi.XRT_MAT_METAL
    t = s.triangles()
    a, b = s.desc.objects[first], s.desc.objects[second]
    assert np.array_equal(t[a.first:a.first + a.count].view(np.uint32), t[b.first:b.first + b.count].view(np.uint32))
    _, cnt, per = wb.reference("twins")
    assert (per["first_obj"] == first).any() and not (per["first_obj"] == second).any()
    assert cnt["whit_rays"] == cnt["samples"]   # every hit resolved to the Lambert twin: no metal child


def test_cover_emitter():
    s = wb.scene("emitter")
    _, cnt, per = wb.reference("emitter")
    emitters = [i for i in range(s.desc.n_objects) if s.desc.objects[i].light >= 0]
    assert len(emitters) == 1 and s.desc.objects[emitters[0]].material == abi.XRT_MAT_NONE
    on_emitter = np.isin(per["first_obj"], emitters)
    assert on_emitter.any() and not per["radiance"][on_emitter].any()
    # the emitter lies between the floor and the point light and does not occlude
    o = np.array([[278.0, 100.0, 279.5]], np.float32)
    d = np.array([[0.0, 1.0, 0.0]], np.float32)
    obj, pos, _, _ = wr.intersect(s, o, d)
    assert obj[0] == emitters[0] and pos[0, 1] == 548.0
    assert not wr.occluded(s, o, d, np.array([448.4], np.float32))[0]
    assert ((per["shadow"] > 0) & (per["shadow_hit"] == 0)).any()


# ---- the level walk against a scalar FIFO, through the mesh ----
@pytest.mark.parametrize("case", ["glass_70", "metal_9"])
def test_level_walk_equals_a_scalar_queue_walk_through_the_mesh(case):
    s = wb.scene(case)
    ro = np.array([wb.NEAR_C2W[12:15]], np.float32)
    rd = wr.normalize(np.array([wb.MESH_CENTER], np.float32) + np.array([[20.0, -15.0, 0.0]], np.float32) - ro)
    depth = wb.CASES[case][4]
    total, cnt, per = wr.integrate(s, ro, rd, depth)
    want, pops = scalar_walk(s, ro[0], rd[0], depth)
    assert per["first_obj"][0] == wb.object_index(s, wb.MESH)
    assert per["rays"][0] == pops and pops > 1
    assert np.array_equal(bits(total[0]), bits(want))
