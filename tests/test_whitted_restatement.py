"""The Whitted checker and the host layers of the feature, without a GPU: the restatement's
geometry against the reference's own geometry.cpp (tests/golden/ref_whitted_kats.json), the
host-scene facade's delta lights and materials, null arguments, what orc_query does with
non-unit and NaN directions, and — scene by scene — the conditions the GPU tests rely on."""
import collections
import ctypes as C
import json
import os

import numpy as np
import pytest

import whitted_restatement as wr
import whitted_scenes as ws
from xraytracer_amd import abi, scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kats():
    with open(os.path.join(ROOT, "tests", "golden", "ref_whitted_kats.json")) as f:
        return json.load(f)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_restatement_geometry_equals_reference(kats):
    vin = np.array(kats["math"]["in"], np.uint32).view(np.float32)
    want = np.array(kats["math"]["out"], np.uint32)
    I, N = vin[:, :3], vin[:, 3:]
    rl, rr = wr.reflect(I, N), wr.refract(I, N)
    got = np.concatenate([rl, rr, wr.fresnel(I, N)[:, None], wr.normalize(rl), wr.normalize(rr)], axis=1)
    assert np.array_equal(bits(got), want), np.argwhere(bits(got) != want)[:5]
    kr = want[:, 6].view(np.float32)
    # the fixture covers both sides of total internal reflection and refract's zero vector
    assert (kr >= 1).any() and (kr < 1).any() and (want[:, 3:6] == 0).all(axis=1).any()


def test_restatement_light_constructors_equal_reference(kats):
    for L in kats["lights"]:
        m = np.array(L["l2w"], np.uint32).view(np.float32)
        assert np.array_equal(bits(wr.point_light_pos(m)), np.array(L["pos"], np.uint32))
        assert np.array_equal(bits(wr.distant_light_dir(m)), np.array(L["dir"], np.uint32))


def test_hscene_delta_lights_and_materials(kats):
    s = scenes.SceneBundle()
    s.add_mesh("a", ws.quad((0, 0, 0), (1, 0, 0), (1, 1, 0), (0, 1, 0)), (0.1, 0.2, 0.3))
    s.add_sphere("b", (0, 0, -3), 1.0, (0.4, 0.5, 0.6))
    s.add_sphere("c", (3, 0, -3), 1.0, (0.7, 0.8, 0.9))
    s.add_sphere("d", (6, 0, -3), 1.0, (0.7, 0.8, 0.9))
    s.set_material("a", "metal")
    s.set_material("b", "glass")
    s.set_material("c", "none")
    s.set_material("d", "glass")
    s.set_material("d", "lambert")   # back again: a Lambert without the old albedo
    for k, L in enumerate(kats["lights"]):   # the two example.cpp matrices first
        m = np.array(L["l2w"], np.uint32).view(np.float32)
        s.add_distant_light(f"d{k}", m, (1.0, 0.5, 0.25), 2.0)
        s.add_point_light(f"p{k}", m, (0.63, 0.33, 0.03), 50.0)
    s.flatten()
    mat = {n: s.desc.objects[i].material for i, n in enumerate(s.object_names())}
    assert mat == {"a": abi.XRT_MAT_METAL, "b": abi.XRT_MAT_GLASS, "c": abi.XRT_MAT_NONE, "d": abi.XRT_MAT_LAMBERT}
    p, n = s.delta_lights()
    assert n == 2 * len(kats["lights"])
    for k, L in enumerate(kats["lights"]):   # push-back order
        d, q = p[2 * k], p[2 * k + 1]
        assert (d.kind, q.kind) == (abi.XRT_DLIGHT_DISTANT, abi.XRT_DLIGHT_POINT)
        assert np.array_equal(bits(d.dir[:]), np.array(L["dir"], np.uint32))
        assert np.array_equal(bits(q.pos[:]), np.array(L["pos"], np.uint32))
        assert (list(d.color), d.intensity) == ([1.0, 0.5, 0.25], 2.0)
        assert q.intensity == 50.0 and np.array_equal(bits(q.color[:]), bits([0.63, 0.33, 0.03]))
    with pytest.raises(abi.XrtError):
        s.set_material("no such object", "metal")


def test_example_scene_lights_are_the_reference_examples(kats):
    p, n = scenes.example(8, 6).delta_lights()
    assert n == 2
    assert np.array_equal(bits(p[0].dir[:]), np.array(kats["lights"][0]["dir"], np.uint32))
    assert np.array_equal(bits(p[1].pos[:]), np.array(kats["lights"][1]["pos"], np.uint32))


def test_null_arguments():
    lib = abi.lib()
    m = np.eye(4, dtype=np.float32).reshape(16)
    c = abi.f3((1, 1, 1))
    s = scenes.SceneBundle()
    assert lib.xrt_set_delta_lights(None, None, 0) == abi.XRT_ERR_INVALID
    assert lib.xrt_test_whitted_math(None, None, 0, None) == abi.XRT_ERR_INVALID
    for fn in (lib.xrt_hscene_add_point_light, lib.xrt_hscene_add_distant_light):
        assert fn(None, b"x", abi.fptr(m), abi.fptr(c), 1.0) == abi.XRT_ERR_INVALID
        assert fn(s.h, None, abi.fptr(m), abi.fptr(c), 1.0) == abi.XRT_ERR_INVALID
        assert fn(s.h, b"x", None, abi.fptr(c), 1.0) == abi.XRT_ERR_INVALID
        assert fn(s.h, b"x", abi.fptr(m), None, 1.0) == abi.XRT_ERR_INVALID
    n = C.c_uint32()
    p = C.POINTER(abi.XrtDeltaLight)()
    assert lib.xrt_hscene_delta_lights(None, C.byref(p), C.byref(n)) == abi.XRT_ERR_INVALID
    assert lib.xrt_hscene_delta_lights(s.h, None, C.byref(n)) == abi.XRT_ERR_INVALID
    assert lib.xrt_hscene_delta_lights(s.h, C.byref(p), None) == abi.XRT_ERR_INVALID
    assert lib.xrt_hscene_set_material(None, b"x", 1) == abi.XRT_ERR_INVALID
    assert lib.xrt_hscene_set_material(s.h, None, 1) == abi.XRT_ERR_INVALID
    s.add_sphere("x", (0, 0, 0), 1.0, (1, 1, 1))
    assert lib.xrt_hscene_set_material(s.h, b"x", 17) == abi.XRT_ERR_INVALID


def test_orc_query_takes_directions_as_given():
    """non-unit: t is the ray parameter (half as large for a doubled direction, same point);
    NaN: no object, for triangles and spheres"""
    s = ws.scene("example")
    o = np.array([[0, 0, 8], [0, 0, 8]], np.float32)
    d = np.array([[0, 0, -1], [0, -1, -1]], np.float32)   # the sphere; the plane
    obj1, pos1, _, _ = wr.intersect(s, o, d)
    obj2, pos2, _, _ = wr.intersect(s, o, d * np.float32(2.0))
    assert (obj1 >= 0).all() and np.array_equal(obj1, obj2) and np.array_equal(pos1, pos2)
    t1 = wr._query(s, o, d)[:, 3]
    t2 = wr._query(s, o, d * np.float32(2.0))[:, 3]
    assert np.array_equal(t1, t2 * np.float32(2.0))
    objn, _, _, _ = wr.intersect(s, o, np.full((2, 3), np.nan, np.float32))
    assert (objn < 0).all()
    assert not wr.occluded(s, o, np.full((2, 3), np.nan, np.float32), np.full(2, wr.FLT_MAX, np.float32)).any()


def scalar_walk(s, ro, rd, max_depth):
    """Src/integrator.h:303-393 for one camera ray as written there: a std::queue (a deque), one
    ray popped at a time, total_radiance added to in pop order.  Returns (radiance, pops)."""
    F = np.float32
    sky = np.array(wr.SKY, F)
    lights = wr.delta_lights(s)
    total, pops = np.zeros(3, F), 0
    rays = collections.deque([(np.asarray(ro, F), np.asarray(rd, F), np.ones(3, F), 0)])
    with np.errstate(all="ignore"):
        while rays:
            o, d, thr, depth = rays.popleft()
            pops += 1
            if depth > max_depth:
                total = total + thr * sky
                continue
            obj, pos, ng, ns = (a[0] for a in wr.intersect(s, o[None], d[None]))
            if obj < 0:
                total = total + thr * sky
                continue
            ob = s.desc.objects[int(obj)]
            if ob.material == abi.XRT_MAT_LAMBERT:
                rad = np.zeros(3, F)
                fr = np.array(ob.albedo[:], F) / F(3.14159265359)
                for kind, lpos, ldir, color, intensity in lights:
                    if kind == abi.XRT_DLIGHT_POINT:
                        ld = lpos - pos
                        dist = wr.length(ld)
                        wi, pdf, tmax = wr.divs(ld, dist), dist * dist, dist
                    else:
                        wi, pdf, tmax = -ldir, F(1.0), wr.FLT_MAX
                    so = pos + wr.muls(ng, F(0.1))
                    vis = F(not wr.occluded(s, so[None], wi[None], np.array([tmax], F))[0])
                    t = wr.muls(fr, vis) * wr.muls(color, intensity)
                    t = wr.muls(t, wr.smax(F(0.0), wr.dot(ns, wi)))
                    rad = rad + wr.divs(t, pdf)
                total = total + rad * thr
            elif ob.material == abi.XRT_MAT_METAL:
                rays.append((pos + wr.muls(ng, F(0.001)), wr.reflect(d, ng), wr.muls(thr, F(0.8)), depth + 1))
            elif ob.material == abi.XRT_MAT_GLASS:
                kr = wr.fresnel(d, ng)
                outside = wr.dot(d, ng) < F(0.0)
                bias = wr.muls(ng, F(0.001))
                t9 = wr.muls(thr, F(0.9))
                if kr < F(1.0):
                    rays.append((pos - bias if outside else pos + bias, wr.normalize(wr.refract(d, ng)),
                                 wr.muls(t9, F(1.0) - kr), depth + 1))
                rays.append((pos + bias if outside else pos - bias, wr.normalize(wr.reflect(d, ng)), wr.muls(t9, kr),
                             depth + 1))
    return total, pops


@pytest.mark.parametrize("case, direction", [("glass_3", (0.3, -0.35, -1.0)), ("glass_3", (-0.35, -0.3, -1.0)),
                                             ("glass_3", (0.0, 0.5, -1.0)), ("mirrors_9", (0.0, -0.2, -1.0)),
                                             ("medium_box", (0.3, -0.15, -1.0))])
def test_level_walk_equals_a_scalar_queue_walk(case, direction):
    """the restatement's level-by-level walk against the reference's loop taken literally — a
    FIFO of single rays — for single samples: same radiance bits, same number of pops"""
    s = ws.scene(case)
    cam = s.camera.c2w.reshape(4, 4)
    ro = cam[3, :3].astype(np.float32)[None]
    rd = wr.normalize((np.array(direction, np.float32) @ cam[:3, :3]).astype(np.float32)[None])
    depth = ws.CASES[case][4]
    total, cnt, per = wr.integrate(s, ro, rd, depth)
    want, pops = scalar_walk(s, ro[0], rd[0], depth)
    assert per["rays"][0] == pops and pops > 1
    assert np.array_equal(bits(total[0]), bits(want))


def test_batching_keeps_a_samples_order():
    """a sample alone and inside a batch gives the same bits: batching never reorders its sum"""
    s = ws.scene("glass_3")
    ro = np.array([[0, 0, 0]], np.float32)
    rd = wr.normalize(np.array([[0.3, -0.35, -1.0]], np.float32))   # towards the glass ball
    total, cnt, per = wr.integrate(s, ro, rd, 3)
    assert cnt["whit_refract"] > 0 and per["rays"][0] > 3
    # the same sample inside a batch gives the same bits: batching never reorders a sample's sum
    ro2 = np.repeat(ro, 3, axis=0)
    rd2 = np.concatenate([wr.normalize(np.array([[0.0, 0.5, -1.0]], np.float32)), rd,
                          wr.normalize(np.array([[-0.4, -0.3, -1.0]], np.float32))])
    total2, _, _ = wr.integrate(s, ro2, rd2, 3)
    assert np.array_equal(bits(total2[1]), bits(total[0]))


# ---- scene coverage: the restatement alone meets the conditions the GPU tests state ----
def test_cover_example_scene():
    for name in ("example", "example_shard", "example_accumulate"):
        _, cnt, per = ws.reference(name)
        assert 0 < per["shadow_hit"].sum() < cnt["shadow_rays"]
    full, shard, acc = (ws.reference(n)[0] for n in ("example", "example_shard", "example_accumulate"))
    assert np.array_equal(shard[1::3], full[1::3]) and not shard[0::3].any() and not shard[2::3].any()
    assert not np.array_equal(acc, full)


def test_cover_stream_crossing():
    for name, spp in (("stream_70", 70), ("stream_330", 330)):
        _, cnt, _ = ws.reference(name)
        assert cnt["draws"] == 2 * cnt["samples"] == 2 * 48 * spp
    assert ws.reference("stream_70")[1]["rng_twists"] == 48 and ws.reference("stream_330")[1]["rng_twists"] == 96


def test_cover_mirror_chain():
    for name in ("mirrors_3", "mirrors_9", "mirrors_0"):
        _, cnt, per = ws.reference(name)
        assert cnt["whit_depth_cut"] > 0
        if name != "mirrors_0":
            assert ((per["rays"] > 1) & (per["shadow"] > 0)).any()
    assert ws.scene("mirrors_3").desc.n_spheres == 0


def test_cover_glass_tree():
    for name in ("glass_3", "glass_max"):
        _, cnt, per = ws.reference(name)
        depth = ws.CASES[name][4]
        assert cnt["whit_refract"] > 0 and cnt["whit_tir"] > 0 and cnt["whit_depth_cut"] > 0
        assert per["cut"].max() == 2 ** (depth + 1)
        assert per["shadow"].sum() > 0   # some paths reach the Lambert floor
    d = ws.scene("glass_3").desc
    assert d.n_spheres > 0 and d.n_tris > 0 and ws.CASES["glass_max"][4] == abi.XRT_WHITTED_MAX_DEPTH


def test_cover_scene_kinds():
    assert ws.scene("cornell_tri").desc.n_spheres == 0 and ws.scene("cornell_tri").desc.n_lights == 0
    for name, n in (("spheres_small", 6), ("spheres_bvh", 21)):
        d = ws.scene(name).desc
        assert d.n_tris == 0 and d.n_spheres == n
        _, cnt, _ = ws.reference(name)
        assert cnt["whit_refract"] > 0 and cnt["whit_depth_cut"] > 0 and cnt["shadow_rays"] > 0


def test_cover_emitter_and_no_material():
    s = ws.scene("cornell_emitter")
    _, cnt, per = ws.reference("cornell_emitter")
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
    lit_floor = (per["shadow"] > 0) & (per["shadow_hit"] == 0)
    assert lit_floor.any()


def test_cover_medium_box():
    s = ws.scene("medium_box")
    _, cnt, per = ws.reference("medium_box")
    boxes = [i for i in range(s.desc.n_objects) if s.desc.objects[i].kind == abi.XRT_OBJ_BOX]
    assert len(boxes) == 1 and s.desc.objects[boxes[0]].material == abi.XRT_MAT_NONE
    assert s.desc.n_tris > 0 and s.desc.n_spheres > 0
    on_box = np.isin(per["first_obj"], boxes)
    assert on_box.any() and not per["radiance"][on_box].any()
    assert (~on_box).any() and cnt["shadow_rays"] > 0 and (per["rays"] > 1).any()


def test_cover_rejection_and_edges():
    _, cnt, _ = ws.reference("rejection")
    assert 0 < cnt["rejected"] < cnt["samples"]
    _, cnt, _ = ws.reference("no_lights")
    assert cnt["shadow_rays"] == 0
