"""The guide-buffer cases, checked without a GPU on the restatement alone
(tests/aov_restatement.py): the frames tests/test_gpu_aov.py compares with the device's really
reach the situations that test relies on."""
import numpy as np
import pytest

import aov_restatement as ar
import whitted_bvh_scenes as wb
import whitted_restatement as wr
from xraytracer_amd import abi

KINDS = ar.LDS_KINDS + tuple("bvh_" + n for n in ar.BVH_KINDS)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def objects_where(s, pred):
    return [i for i in range(s.desc.n_objects) if pred(s.desc.objects[i])]


def test_abi_constants():
    assert abi.XRT_SCHED_AOV == 8 and abi.XRT_ABI_VERSION == 14
    assert ar.PLANES == ("albedo", "normal", "depth", "alpha", "object")
    assert [f for f, _ in abi.XrtAovBuffers._fields_] == list(ar.PLANES)


@pytest.mark.parametrize("name", sorted(ar.CASES))
def test_every_plane_is_finite(name):
    planes, cnt, per = ar.reference(name)
    for k in ("albedo", "normal", "depth", "alpha"):
        assert np.isfinite(planes[k]).all(), k
    assert np.isfinite(per["val"]).all()
    _, w, h, spp, _ = ar.CASES[name]
    assert cnt["samples"] == cnt["path_slots"] * spp and cnt["draws"] == 2 * cnt["samples"]


def test_all_miss_and_all_hit_pixels():
    planes, _, per = ar.reference("example")
    hits = (per["obj"] >= 0).sum(axis=1)
    assert (hits == 0).any() and (hits == 3).any()
    assert (planes["alpha"] == 0).any() and (planes["alpha"] == 1).any()
    # an all-miss pixel is +0.0f in every float channel and -1 in object
    miss = planes["alpha"] == 0
    for k in ("albedo", "normal", "depth"):
        assert not bits(planes[k][miss]).any()
    assert (planes["object"][miss] == -1).all()


def test_samples_on_different_objects():
    """a pixel whose samples land on two objects: its albedo mean lies strictly between theirs"""
    s = ar.scene("example")
    planes, _, per = ar.reference("example")
    obj = per["obj"]
    two = np.array([len(set(o[o >= 0])) > 1 for o in obj])
    assert two.any()
    lo = min(s.desc.objects[i].albedo[0] for i in range(s.desc.n_objects))
    hi = max(s.desc.objects[i].albedo[0] for i in range(s.desc.n_objects))
    n = int(np.argmax(two & (obj >= 0).all(axis=1)))
    assert two[n] and (obj[n] >= 0).all()
    i, j = per["pix"][n]
    assert lo < planes["albedo"][i, j, 0] < hi


def test_sample_zero_misses_and_a_later_one_hits():
    found = []
    for name in sorted(ar.CASES):
        planes, _, _ = ar.reference(name)
        if ((planes["object"] == -1) & (planes["alpha"] > 0)).any():
            found.append(name)
    assert found
    # ... among them a case of more than one window
    _, _, per = ar.reference("edge_330")
    o = per["obj"]
    assert ((o[:, 0] < 0) & (o[:, 1:] >= 0).any(axis=1)).any()


def test_partial_coverage_gives_fractional_alpha():
    planes, _, _ = ar.reference("edge_330")
    a = planes["alpha"]
    assert ((a > 0) & (a < 1)).any()


def test_metal_and_glass_first_hits():
    for name, mat in (("mirrors_3", abi.XRT_MAT_METAL), ("glass_3", abi.XRT_MAT_GLASS), ("bvh_glass", abi.XRT_MAT_GLASS)):
        s = ar.scene(name)
        planes, _, per = ar.reference(name)
        ids = objects_where(s, lambda o: o.material == mat)
        on = np.isin(per["obj"], ids)
        assert on.any(), name
        assert (per["val"][on][:, 0:3] == 1.0).all()
        # a pixel whose samples all hit such an object has albedo exactly (1, 1, 1)
        full = on.all(axis=1)
        assert full.any(), name
        i, j = per["pix"][int(np.argmax(full))]
        assert (planes["albedo"][i, j] == 1.0).all()


def test_emitter_first_hit():
    s = ar.scene("cornell_emitter")
    _, _, per = ar.reference("cornell_emitter")
    ids = objects_where(s, lambda o: o.light >= 0)
    assert ids and all(s.desc.objects[i].material == abi.XRT_MAT_NONE for i in ids)
    on = np.isin(per["obj"], ids)
    assert on.any()
    v = per["val"][on]
    assert not v[:, 0:3].any() and (v[:, 7] == 1.0).all() and (v[:, 6] > 0).all()


def test_medium_box_first_hit():
    s = ar.scene("medium_box")
    _, _, per = ar.reference("medium_box")
    ids = objects_where(s, lambda o: o.kind == abi.XRT_OBJ_BOX)
    on = np.isin(per["obj"], ids)
    assert on.any()
    v = per["val"][on]
    assert not v[:, 0:3].any() and (v[:, 7] == 1.0).all()


def test_lambert_albedo_is_the_uploaded_one():
    s = ar.scene("cornell_tri")
    _, _, per = ar.reference("cornell_tri")
    obj, val = per["obj"].reshape(-1), per["val"].reshape(-1, 8)
    seen = 0
    for i in objects_where(s, lambda o: o.material == abi.XRT_MAT_LAMBERT):
        m = obj == i
        if m.any():
            seen += 1
            assert (bits(val[m][:, 0:3]) == bits(np.array(s.desc.objects[i].albedo[:], np.float32))).all()
    assert seen >= 3


def test_bvh_cases_are_beyond_lds_and_ties_resolve_by_object_order():
    for n in ar.BVH_KINDS:
        s = ar.scene("bvh_" + n)
        assert s.desc.n_tris > 1024 and s.desc.n_spheres == 0 and s.desc.n_boxes == 0
    before, after = ar.scene("bvh_tie_before"), ar.scene("bvh_tie_after")
    ib, ia = wb.object_index(before, before.tie_name), wb.object_index(after, after.tie_name)
    assert (ar.reference("bvh_tie_before")[2]["obj"] == ib).any()
    assert not (ar.reference("bvh_tie_after")[2]["obj"] == ia).any()
    tw = ar.scene("bvh_twins")
    first, second = (wb.object_index(tw, n) for n in tw.twin_order)
    o = ar.reference("bvh_twins")[2]["obj"]
    assert (o == first).any() and not (o == second).any()


def test_edge_cases_cover_windows_and_ring_blocks():
    assert ar.EDGE_SPP == (1, 63, 64, 65, 130, 330)
    assert 2 * 330 > 624   # past one 624-word block of the stream


def test_shard_rows():
    planes, cnt, per = ar.reference("example_shard")
    rows = sorted({i for i, _ in per["pix"]})
    assert rows == list(range(1, 36, 3)) and cnt["path_slots"] == 12 * 48
    other = np.ones(36, bool)
    other[rows] = False
    assert not bits(planes["albedo"][other]).any() and not bits(planes["depth"][other]).any()
    assert (planes["object"][other] == -1).all()
    full = ar.reference("example")[0]
    for k in ar.PLANES:
        assert np.array_equal(planes[k][rows], full[k][rows])


@pytest.mark.parametrize("name", ["example", "edge_65"])
def test_rays_are_the_whitted_restatements(name, monkeypatch):
    """every sample's camera ray, sample 0's included, is bit for bit the ray the Whitted
    restatement hands WhittedIntegrator::integrate for the same pixel and sample"""
    _, w, h, spp, _ = ar.CASES[name]
    seen = {}

    def capture(scene, ro, rd, max_depth, lights=None):
        seen["ro"], seen["rd"] = np.array(ro, np.float32), np.array(rd, np.float32)
        return np.zeros((len(ro), 3), np.float32), {}, {}

    monkeypatch.setattr(wr, "integrate", capture)
    wr.render(ar.scene(name), w, h, spp, max_depth=0)
    _, _, per = ar.reference(name)
    assert np.array_equal(bits(seen["ro"]), bits(per["ro"].reshape(-1, 3)))
    assert np.array_equal(bits(seen["rd"]), bits(per["rd"].reshape(-1, 3)))
    assert np.array_equal(bits(seen["rd"].reshape(-1, spp, 3)[:, 0]), bits(per["rd"][:, 0]))


def test_refused_scene_has_no_triangle_bvh():
    s = wb.mixed_beyond_lds(24, 18)
    assert s.desc.n_spheres == 1 and s.desc.n_tris > 1024
