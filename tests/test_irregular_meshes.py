"""tests/irregular_meshes.py's scenes and ray sets hold what tests/test_gpu_irregular.py relies on,
shown on the oracle alone (no GPU): enough rays hit and enough miss, the hits are spread over many
triangles and, for the spirals, over many octaves of triangle size, the occluded query has both
outcomes, and no collinear or zero-edge triangle is ever reported.  These are conditions on the
inputs, not on the device."""
import numpy as np
import pytest

import irregular_meshes as im

QUERY_CASES = im.CASES + ("spheres_irregular",)


def family_index(name, hits):
    """per ray the index of the hit triangle in the family's own order, -1 where the ray misses the mesh"""
    s = im.scene(name)
    names = s.object_names()
    base = {names.index(n): 250 * i for i, n in enumerate(s.mesh_names)}
    return np.array([base[h.object] + h.primitive if h.hit and h.object in base else -1 for h in hits])


@pytest.mark.parametrize("name", QUERY_CASES)
def test_ray_set(name):
    rays, tmax = im.rays(name)
    assert len(rays) <= 4000 and rays.dtype == np.float32 and np.all(np.isfinite(rays))
    hits, occ = im.reference(name)
    n = len(rays)
    n_hit = sum(h.hit for h in hits)
    assert n_hit >= n // 4 and n - n_hit >= n // 4, (n_hit, n)
    assert n // 10 <= sum(occ) <= n - n // 10, sum(occ)
    if name == "spheres_irregular":
        assert len({h.object for h in hits if h.hit}) >= 30
        return
    family = name.rsplit("-", 1)[0]
    v, kind = im.triangles(family)
    idx = family_index(name, hits)
    on_mesh = np.unique(idx[idx >= 0])
    assert not np.any(np.isin(kind[on_mesh], (2, 3))), on_mesh[np.isin(kind[on_mesh], (2, 3))]
    usable = int(np.count_nonzero(im.hittable(v)))
    if usable >= 100:
        assert len({(h.object, h.primitive) for h in hits if h.hit}) >= 100
        assert len(on_mesh) >= 100
    else:   # the node-count strips' zero-edge filler aside, every triangle the mesh has
        assert len(on_mesh) >= min(usable, 3)
    if family in im.SPIRALS:
        size = np.ptp(v, axis=1).max(axis=1)[on_mesh]
        assert np.log2(size.max() / size.min()) >= 12.0
    if family == "clumps":
        assert np.any(kind[on_mesh] == 1)        # slivers are hit
        assert np.count_nonzero(kind == 2) >= 20 and np.count_nonzero(kind == 3) >= 5


@pytest.mark.parametrize("name", im.CASES)
def test_scene_takes_the_path_it_is_for(name):
    c = im.culls(name)
    v, kind = im.triangles(name.rsplit("-", 1)[0])
    assert c.bvh and not c.small and c.two_level == name.endswith("-two")
    mesh = im.mesh_triangles(name)
    assert len(mesh) == len(v)
    # the triangles left out of the BVH are the zero-edge ones of the family, and only they
    assert np.array_equal(c.tri_dropped[mesh], kind == 3)
    assert np.all(c.tri_in_bvh[mesh] == (kind != 3))
    # collinear triangles stay in: non-zero edges
    assert np.all(c.tri_in_bvh[mesh][kind == 2])


def test_concentric_boxes_share_their_centre():
    lo, hi, _, _ = im.boxes("concentric-two")
    c = (np.float32(0.5) * (lo + hi).astype(np.float32)).astype(np.float32)     # build_bvh's centroid
    assert np.all(c == c[0])


def test_collinear_triangles_are_exactly_collinear():
    v, kind = im.triangles("clumps")
    co = v[kind == 2]
    e1, e2 = (co[:, 1] - co[:, 0]).astype(np.float32), (co[:, 2] - co[:, 0]).astype(np.float32)
    assert len(co) >= 20
    # one non-zero component each, the same one: e1 . (d x e2) is an exact 0 whatever d is
    assert np.all(np.count_nonzero(e1, axis=1) == 1) and np.all(np.count_nonzero(e2, axis=1) == 1)
    assert np.all((e1 != 0) == (e2 != 0))


def test_sphere_scene_gets_the_threaded_bvh():
    c = im.culls("spheres_irregular")
    assert c.sphere_bvh and c.kind == "sphere" and len(c.sph_lo) >= 16


def test_bvh_info_checks_its_arguments():
    """xrt_test_bvh_info refuses a null context or output before it touches a device"""
    import ctypes as C

    from xraytracer_amd import abi

    out = (C.c_int32 * 8)()
    assert abi.lib().xrt_test_bvh_info(None, out) == abi.XRT_ERR_INVALID
    assert abi.lib().xrt_test_bvh_info(None, None) == abi.XRT_ERR_INVALID


@pytest.mark.parametrize("name", [n for n in im.TOP_CASES if "counts" in n])
def test_camera_rays_fall_on_every_part_of_the_strip(name):
    """the renders of the node-count scenes walk the whole tree: of 16 equal parts of the strip, each
    has a triangle that a camera sample of the 24 x 18 x 2 render hits first"""
    import aov_restatement as ar
    import pyoracle

    s = im.scene(name)
    _, ro, rd = ar.camera_rays(s, im.W, im.H, 2, list(range(im.H)))
    hits = pyoracle.query(s, np.concatenate([ro.reshape(-1, 3), rd.reshape(-1, 3)], axis=1))
    idx = family_index(name, hits)
    n = int(np.count_nonzero(im.triangles(name.rsplit("-", 1)[0])[1] == 0))
    parts = np.unique(idx[(idx >= 0) & (idx < n)] * 16 // n)
    assert len(parts) == 16, parts


def test_camera_rays_hit_the_one_leaf_mesh():
    import aov_restatement as ar
    import pyoracle

    s = im.scene("one_leaf-two")
    _, ro, rd = ar.camera_rays(s, im.W, im.H, 2, list(range(im.H)))
    hits = pyoracle.query(s, np.concatenate([ro.reshape(-1, 3), rd.reshape(-1, 3)], axis=1))
    assert set(family_index("one_leaf-two", hits)) >= {0, 1, 2}
