"""The scenes of the Whitted BVH tests (XRT_FLAG_WHITTED_BVH, k_whitted_bvh) — a helper, not a
test file.  They are the smallest triangle scenes that do not fit the LDS scene carve and reach
each path of the kernel: two-level scenes (the Cornell box's small objects beside a SphereMesh
of more than kLargeObjTris triangles) and one-level scenes (only large meshes; only medium
ones).  Each CASE is rendered by the restatement (tests/whitted_restatement.py, a linear scan
over every triangle) once per session; tests/test_whitted_bvh_restatement.py checks without a
GPU that the restatement alone meets the conditions the GPU test of that scene relies on."""
import functools

import numpy as np

from xraytracer_amd import scenes

import whitted_restatement as wr
import whitted_scenes as ws

MESH = "sphere_mesh"
MESH_CENTER, MESH_RADIUS = (150.0, 420.0, 400.0), 90.0   # scenes.cornell_spheremesh
# the Cornell camera's orientation from 300 in front of the mesh: the mesh is ten pixels wide at 24 x 18
NEAR_C2W = (-1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, -1.0, 0, 150.0, 420.0, 100.0, 1)


def object_index(s, name):
    return s.object_names().index(name)


def add_point(s, emitter=False):
    """ws.cornell_point's point light: inside the box, or (emitter) between the quad emitter and
    the ceiling, so every shadow ray from below crosses the emitter"""
    if emitter:
        s.add_point_light("PointLight", ws.translate(278.0, 548.4, 279.5), (1.0, 1.0, 1.0), 2.0e5)
    else:
        s.add_point_light("PointLight", ws.translate(278.0, 400.0, 279.5), (1.0, 0.95, 0.9), 1.0e5)


def cornell_mesh(w, h, material="glass", n=24, emitter=False, near=False):
    """scenes.cornell_spheremesh (the Cornell box, its quad emitter, a SphereMesh of 2 n^2
    triangles) with a point light and the mesh re-tagged: a two-level scene from n = 24 on"""
    s = scenes.cornell_spheremesh(w, h, n_theta=n, n_phi=n)
    add_point(s, emitter)
    if material != "lambert":
        s.set_material(MESH, material)
    s.flatten()
    if near:
        s.camera = scenes.pinhole(NEAR_C2W, 60.0, w, h)
    s.integrator, s.max_depth = "whitted", 3
    return s


def pinned(w, h):
    """the scene tests/test_gpu_whitted.py::test_two_level_scene_is_unsupported refuses without
    the flag"""
    s = scenes.cornell_spheremesh(w, h, n_theta=40, n_phi=40)
    s.add_point_light("PointLight", ws.translate(278.0, 400.0, 279.5), (1.0, 1.0, 1.0), 1.0e5)
    s.flatten()
    s.integrator = "whitted"
    return s


def visible_mesh_triangle(s):
    """(global triangle index, its three vertices [3, 3]) of the mesh triangle the ray from the
    NEAR camera to the mesh centre hits"""
    o = np.array([NEAR_C2W[12:15]], np.float32)
    d = wr.normalize(np.array([MESH_CENTER], np.float32) - o)
    h = wr._query(s, o, d)
    obj, prim = int(h[0, 1:2].view(np.int32)[0]), int(h[0, 2:3].view(np.int32)[0])
    assert obj == object_index(s, MESH)
    tri = s.desc.objects[obj].first + prim
    return tri, s.triangles()[tri]


def tie(w, h, before):
    """cornell_mesh(metal) plus a one-triangle Lambert mesh whose vertices are bitwise those of
    a camera-visible mesh triangle: both are hit at the same t, and Scene::intersect keeps the
    one that comes first in object order — the copy (before) or the mesh (after).  The object
    order is the host scene's unordered_map order, so the copy's name is chosen for the side."""
    _, verts = visible_mesh_triangle(cornell_mesh(w, h, "metal", near=True))
    for k in range(64):
        name = f"tie_{k:02d}"
        s = scenes.cornell_spheremesh(w, h, n_theta=24, n_phi=24)
        add_point(s)
        s.set_material(MESH, "metal")
        s.add_mesh(name, verts.reshape(1, 9), (0.8, 0.3, 0.2))
        s.flatten()
        if (object_index(s, name) < object_index(s, MESH)) == before:
            s.camera = scenes.pinhole(NEAR_C2W, 60.0, w, h)
            s.integrator, s.max_depth = "whitted", 3
            s.tie_name = name
            return s
    raise AssertionError("no name puts the copy on the wanted side of the mesh")


def twins(w, h):
    """the same 24 x 24 SphereMesh twice at one place, the first in object order Lambert, the
    second metal: every triangle of one ties with its twin inside the BVH, and the first wins"""
    s = scenes.SceneBundle()
    s.load_obj(scenes.CORNELL_OBJ)
    s.add_quad_light("QuadLight", (343.0, 548.0, 227.0), (343.0, 548.0, 332.0), (213.0, 548.0, 227.0), (25.0, 25.0, 25.0))
    for name in ("twin_a", "twin_b"):
        s.add_sphere_mesh(name, MESH_CENTER, MESH_RADIUS, 24, 24, (0.58, 0.58, 0.58))
    add_point(s)
    s.flatten()
    order = sorted(("twin_a", "twin_b"), key=lambda n: object_index(s, n))
    s.set_material(order[1], "metal")
    s.flatten()
    s.camera = scenes.pinhole(NEAR_C2W, 60.0, w, h)
    s.integrator, s.max_depth = "whitted", 3
    s.twin_order = order
    return s


def big_meshes(w, h):
    """only large meshes: a Lambert SphereMesh as ground and a glass one on top of it, one
    distant light; no small objects, so a one-level scene with every triangle in the BVH"""
    s = scenes.SceneBundle()
    s.add_sphere_mesh("ground", (0.0, -50.0, -6.0), 50.0, 24, 24, (0.5, 0.55, 0.5))
    s.add_sphere_mesh("ball", (0.0, 0.9, -6.0), 1.0, 24, 24, (0, 0, 0))
    s.set_material("ball", "glass")
    s.add_distant_light("DistantLight", scenes.EXAMPLE_DISTANT_L2W, (1.0, 1.0, 1.0), 1.0)
    s.flatten()
    s.camera = scenes.pinhole(ws.IDENT + (0, 1.2, 0, 1), 60.0, w, h)
    s.integrator, s.max_depth = "whitted", 3
    return s


def medium_meshes(w, h, n=6):
    """n SphereMeshes of 12 x 10 (240 triangles each: none above kLargeObjTris) with mixed
    materials over a quad floor: more than kSmallTris triangles in all, no large object, so a
    one-level scene whose BVH holds every triangle"""
    s = scenes.SceneBundle()
    s.add_mesh("floor", ws.quad((-6, -0.5, 0), (6, -0.5, 0), (6, -0.5, -12), (-6, -0.5, -12)), (0.6, 0.6, 0.55))
    for k in range(n):
        x, z = -2.4 + 2.4 * (k % 3), -5.0 - 2.2 * (k // 3)
        s.add_sphere_mesh(f"m{k}", (x, 0.3, z), 0.8, 12, 10, (0.3 + 0.1 * k, 0.5, 0.4))
        if k % 3 == 1:
            s.set_material(f"m{k}", "metal")
        elif k % 3 == 2:
            s.set_material(f"m{k}", "glass")
    s.add_distant_light("DistantLight", scenes.EXAMPLE_DISTANT_L2W, (1.0, 1.0, 1.0), 1.0)
    s.add_point_light("PointLight", ws.translate(0.0, 4.0, -5.0), (0.9, 0.8, 0.6), 40.0)
    s.flatten()
    s.camera = scenes.pinhole(ws.IDENT + (0, 1.0, 1.0, 1), 60.0, w, h)
    s.integrator, s.max_depth = "whitted", 3
    return s


# name -> (scene builder, width, height, spp, max_depth, render keywords); ws.CASES' layout
CASES = {
    "glass": (lambda: cornell_mesh(24, 18, "glass"), 24, 18, 2, 3, {}),
    "pinned": (lambda: pinned(24, 18), 24, 18, 2, 3, {}),
    "metal_9": (lambda: cornell_mesh(24, 18, "metal"), 24, 18, 2, 9, {}),
    "big_meshes": (lambda: big_meshes(24, 18), 24, 18, 2, 3, {}),
    "medium_meshes": (lambda: medium_meshes(24, 18), 24, 18, 2, 3, {}),
    "tie_before": (lambda: tie(24, 18, True), 24, 18, 2, 3, {}),
    "tie_after": (lambda: tie(24, 18, False), 24, 18, 2, 3, {}),
    "twins": (lambda: twins(24, 18), 24, 18, 2, 3, {}),
    "emitter": (lambda: cornell_mesh(24, 18, "glass", emitter=True), 24, 18, 2, 3, {}),
    "glass_shard": (lambda: cornell_mesh(24, 18, "glass"), 24, 18, 2, 3, dict(shard_index=1, shard_count=3)),
    "glass_accumulate": (lambda: cornell_mesh(24, 18, "glass"), 24, 18, 2, 3, dict(initial=True)),
    "glass_70": (lambda: cornell_mesh(8, 6, "glass", near=True), 8, 6, 70, 3, {}),
}


@functools.lru_cache(maxsize=None)
def scene(name):
    return CASES[name][0]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(frame, counters, per-sample record) of the restatement for CASES[name]; computed once"""
    _, w, h, spp, depth, kw = CASES[name]
    kw = dict(kw)
    if kw.pop("initial", False):
        kw["initial"] = ws.initial_image(w, h)
    img, cnt, per = wr.render(scene(name), w, h, spp, max_depth=depth, **kw)
    img.setflags(write=False)
    return img, cnt, per


def mixed_beyond_lds(w, h):
    """the smallest scene at test size with no triangle BVH that exceeds the LDS scene carve: one
    24 x 24 SphereMesh (1,152 triangles at 112 B each in step_layout: 129 KB against kStepLds =
    64 KiB) and one Sphere, which makes the scene mixed — and only triangle scenes get a BVH"""
    s = scenes.SceneBundle()
    s.add_sphere_mesh("ball_mesh", (0.0, 0.0, -6.0), 1.0, 24, 24, (0.5, 0.5, 0.5))
    s.add_sphere("ball", (2.5, 0.0, -6.0), 1.0, (0.5, 0.5, 0.5))
    s.add_distant_light("DistantLight", scenes.EXAMPLE_DISTANT_L2W, (1.0, 1.0, 1.0), 1.0)
    s.flatten()
    s.camera = scenes.pinhole(ws.IDENT + (0, 0, 0, 1), 60.0, w, h)
    s.integrator, s.max_depth = "whitted", 3
    return s
