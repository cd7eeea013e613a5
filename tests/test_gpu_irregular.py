"""The kernels that walk a hierarchy, on the irregular meshes of tests/irregular_meshes.py: trees at the
walks' stack limits, trees no upload accepted before build_bvh_fit, median-only and lopsided trees,
trees of 63, 64 and 65 nodes around the LDS-resident top, a one-leaf root, and a threaded sphere BVH
over nested spheres.  Everything is compared bit for bit: xrt_query with the oracle's restatement of
Scene::intersect / Scene::occluded, GI and Direct frames and their counters with the oracle's render,
Whitted frames and the guide planes with their restatements (linear scans over every triangle).
xrt_test_bvh_info shows that each scene reached the edge it was built for, with the figures the host
program (tests/cpp/bvh_kat.cpp) prints for the same boxes.  tests/test_irregular_meshes.py proves on
the CPU that the ray sets hit what they are aimed at.

Why the scenes at the limits are legal inputs: the host program finds that the stack of a ray that
overlaps every box never holds more than depth + 1 resp. 3 * depth4 + 1 entries, in either child
order.  bvh_trace (bvh_walk.h; k_trace_bvh, and through WhitBvh of whit_trace.h k_whitted_bvh and
k_aov_bvh) indexes stk[sp * STRIDE] with sp below bvh_stack, the size the launchers reserve
(BvhLds::bytes(P.bvh_stack, ...)); k_trace_deep4 and k_trace_deep4q (trace.hip) index below
bvh4_stack in the same way; the wave's quad stacks (wave_deep.h) are circular over kQs = 64 >=
kBvh4Stack entries.

Which kernel reads which tree: the binary tree of a one-level scene is walked by every kernel
(k_trace_bvh for queries and the wavefront schedule).  Of a two-level scene, queries and the path
integrators walk the 4-wide form; only k_whitted_bvh and k_aov_bvh walk its binary tree.  So the
trees around kBvhTopNodes (`node < ntop` in bvh_trace: 63 and 64 nodes lie in LDS whole, the 65th is
read from memory) and the one-leaf root with its empty right child are walked in both ways: the
allcounts_N scenes by test_query, the counts_N and one_leaf scenes by test_whitted_glass and
test_guide_planes, each with its node count asserted."""
import numpy as np
import pytest

import aov_restatement as ar
import irregular_meshes as im
import pyoracle
import whitted_restatement as wr
import whitted_scenes as ws
from gpu_checks import assert_frame, assert_same_bits, counters_equal, render_pair, renderer  # noqa: F401
from test_gpu_query import record
from xraytracer_amd import abi
from xraytracer_amd.renderer import HipRenderer

pytestmark = pytest.mark.gpu

QUERY_CASES = im.CASES + ("spheres_irregular",)
LIMITS = im.limits()


@pytest.fixture(scope="module")
def host_records(tmp_path_factory):
    """what the host program prints for every scene's boxes (plain build, one run)"""
    d = tmp_path_factory.mktemp("bvh_kat")
    return im.run_program(d, im.box_files(d))


def check_info(info, rec, name):
    """xrt_test_bvh_info of an uploaded scene against the host program's record of its boxes"""
    r = {k: int(v) for k, v in rec.items() if k not in ("first", "fnv")}
    if name == "spheres_irregular":
        assert info["n_snode"] == r["skip"] and info["bvh_nodes"] == info["bvh4_nodes"] == info["two_level"] == 0
        return
    two = name.endswith("-two")
    assert info["two_level"] == two and info["n_snode"] == 0
    assert info["bvh_nodes"] == r["nodes"] and info["bvh_stack"] == r["depth"] + 1 <= LIMITS["KAT_STACK"]
    assert info["bvh_tris"] == r["n"]
    if two:
        assert info["bvh4_nodes"] == r["nodes4"] and info["bvh4_stack"] == 3 * r["depth4"] + 1 <= LIMITS["KAT_STACK4"]
    else:
        assert info["bvh4_nodes"] == info["bvh4_stack"] == 0
    assert info["stack_entry"] == 2        # every tree here has at most 0x10000 nodes
    e = im.EDGES.get(name, {})
    if e.get("fits", True):                # the first build, so the edge the scene was tuned to
        if "depth" in e:
            assert info["bvh_stack"] == e["depth"] + 1
        if "depth4" in e:
            assert info["bvh4_stack"] == 3 * e["depth4"] + 1
        if "nodes" in e:
            assert info["bvh_nodes"] == e["nodes"]


def test_edges_are_reached(renderer, host_records):
    """the scenes at the limits report them, and the scenes refused before build_bvh_fit upload"""
    info = {name: renderer.bvh_info(im.scene(name)) for name in QUERY_CASES}     # a refused upload raises
    for name in QUERY_CASES:
        check_info(info[name], host_records[name], name)
    assert info["spiral_38d-one"]["bvh_stack"] == LIMITS["KAT_STACK"]
    assert 43 <= info["spiral_22x-two"]["bvh4_stack"] <= LIMITS["KAT_STACK4"]
    assert [info[f"counts_{n}-two"]["bvh_nodes"] for n in (63, 64, 65)] == [63, 64, 65]
    assert [info[f"allcounts_{n}-one"]["bvh_nodes"] for n in (63, 64, 65)] == [63, 64, 65]
    assert info["one_leaf-two"]["bvh_nodes"] == 1 and info["one_leaf-two"]["bvh_tris"] == 3
    for name, e in im.EDGES.items():
        if not e["fits"]:                  # rebuilt with fewer SAH levels
            assert host_records[name]["first"] != host_records[name]["fnv"]


def test_info_needs_a_scene():
    import ctypes as C

    r = HipRenderer(1)
    try:
        out = (C.c_int32 * 8)()
        assert abi.lib().xrt_test_bvh_info(r.ctx, out) == abi.XRT_ERR_STATE
        assert abi.lib().xrt_test_bvh_info(r.ctx, None) == abi.XRT_ERR_INVALID
    finally:
        r.close()


@pytest.mark.parametrize("name", QUERY_CASES)
def test_query(renderer, name):
    s = im.scene(name)
    rays, tmax = im.rays(name)
    ref, ref_occ = im.reference(name)
    got = renderer.query(s, rays)
    bad = [k for k in range(len(rays)) if not np.array_equal(record(got[k]), record(ref[k]))]
    assert not bad, (name, len(bad), bad[:5], rays[bad[0]])
    got = renderer.query(s, rays, tmax=tmax, occluded=True)
    assert [h.hit for h in got] == ref_occ


# ------------------------------------------------------------------ renders ----
RENDER_FAMILIES = ("spiral_38d", "spiral_22x", "spiral_50d")
RENDER_CASES = tuple(f"{f}-{form}" for f in RENDER_FAMILIES for form in ("one", "two"))
# the scenes whose binary tree k_whitted_bvh and k_aov_bvh walk: the spirals, and the trees around kBvhTopNodes
BINARY_WALK_CASES = RENDER_CASES + im.TOP_CASES
SPP = 2


def assert_top_nodes(r, s, name):
    """a case around kBvhTopNodes was rendered over the tree it is named for"""
    want = im.EDGES[name].get("nodes") if name in im.TOP_CASES else None
    if want is not None:
        assert r.bvh_info(s)["bvh_nodes"] == want


@pytest.fixture(scope="module")
def gi_reference():
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = pyoracle.render(im.scene(name), im.W, im.H, SPP, integrator="gi", max_depth=3)
            cache[name][0].setflags(write=False)
        return cache[name]
    return get


@pytest.mark.parametrize("name", RENDER_CASES)
@pytest.mark.parametrize("sched,deep", [("wavefront", "single"), ("wavefront", "quad"), ("auto", "auto")])
def test_gi(renderer, gi_reference, name, sched, deep):
    """GI through the wavefront schedule with the deep rays walked by one lane and by four, and through
    the schedule the library chooses: for a two-level scene the fused one, with the wave's quad stacks"""
    img, ref, st, g = render_pair(renderer, im.scene(name), im.W, im.H, SPP, ref=gi_reference(name), integrator="gi",
                                  max_depth=3, schedule=sched, deep=deep)
    if sched == "wavefront":
        assert g.schedule == abi.XRT_SCHED_WAVEFRONT
    elif name.endswith("-two"):
        assert g.schedule == abi.XRT_SCHED_STEP_BVH
    assert_frame(img, ref)
    counters_equal(g, st)


@pytest.mark.parametrize("name", BINARY_WALK_CASES)
def test_whitted_glass(name):
    """WhittedIntegrator with the mesh as glass through k_whitted_bvh (XRT_FLAG_WHITTED_BVH)"""
    s = im.scene(name, "glass")
    ref, cnt, _ = wr.render(s, im.W, im.H, SPP, max_depth=3)
    r = HipRenderer(SPP)
    try:
        img = r.render(s, im.W, im.H, max_depth=3, whitted_bvh=True)
        st = r.stats
        assert st.schedule == abi.XRT_SCHED_WHITTED_BVH
        assert_top_nodes(r, s, name)
        assert {k: int(getattr(st, k)) for k in ws.COUNTERS} == {k: int(cnt[k]) for k in ws.COUNTERS}
        assert_frame(img, ref)
    finally:
        r.close()


@pytest.mark.parametrize("name", BINARY_WALK_CASES)
def test_guide_planes(name):
    """xrt_render_aov through k_aov_bvh"""
    s = im.scene(name)
    ref, cnt, _ = ar.render(s, im.W, im.H, SPP)
    r = HipRenderer(SPP)
    try:
        got = r.render_aov(s, im.W, im.H)
        assert_top_nodes(r, s, name)
        assert {k: int(getattr(r.stats, k)) for k in ar.COUNTERS} == {k: int(cnt[k]) for k in ar.COUNTERS}
        for k in ar.PLANES:
            assert_same_bits(got[k], ref[k], k)
    finally:
        r.close()


@pytest.mark.parametrize("schedule,want", [("step", abi.XRT_SCHED_STEP), ("auto", abi.XRT_SCHED_PIXEL)])
def test_spheres_direct(renderer, schedule, want):
    """Direct over the nested spheres through the fused schedule (the threaded BVH in LDS) and through
    the pixel-parallel one"""
    s = im.scene("spheres_irregular")
    img, ref, st, g = render_pair(renderer, s, im.W, im.H, 4, integrator="direct", max_depth=1, schedule=schedule)
    assert g.schedule == want
    assert_frame(img, ref)
    counters_equal(g, st)
