"""The device's camera lists (k_camlist, xraytracer_amd/csrc/spec.hip, read back through
xrt_test_camlist) against their restatement, and the frames rendered from them against the oracle.

k_step_spec takes a successor sample's first hit from the pixel's camera list alone: the closest
of the listed triangles, or — where one triangle is left and covers the pixel — that triangle
untested.  tests/test_camlist_restatement.py proves the restated lists against the oracle
without a GPU; here
  lists     the device's four words per slot equal the restatement's, bit for bit, on every
            scene of tests/camlist_scenes.py and on a row shard: the device is the thing restated,
            so equality is the bar;
  frames    every adversarial scene renders bit for bit as the oracle, with equal counters, when
            every step launch is speculative (16 and 4 slots per wave) — after the lists read
            back from the device have been shown to hold the pixels the scene is for (covered,
            culled, tied ...: camlist_scenes.check_classes over lists equal to the device's);
  boundary  the 64-triangle scene takes the speculative launches, with one triangle more none;
  refusals  no lists without a scene, for spheres, or for 65 triangles.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pyoracle
from gpu_checks import assert_frame, assert_same_bits, counters_equal, render_pair, renderer  # noqa: F401
from xraytracer_amd import abi, scenes
from xraytracer_amd.renderer import HipRenderer

import camlist_restatement as cr
import camlist_scenes as cs

pytestmark = pytest.mark.gpu

SPP = 24


@functools.lru_cache(maxsize=None)
def restated(name):
    """(scene, restated lists) of a case, its preconditions checked — once per module"""
    case = cs.CASES[name]
    scene = case.build()
    lists = cr.camera_lists(scene, case.width, case.height)
    cs.check_classes(name, lists)
    return scene, lists


@functools.lru_cache(maxsize=None)
def oracle_frame(name):
    case = cs.CASES[name]
    return pyoracle.render(restated(name)[0], case.width, case.height, SPP)


def device_lists(r, name):
    """the device's lists of a case, shown equal to the restatement's"""
    case = cs.CASES[name]
    scene, lists = restated(name)
    got = r.camlist(scene, case.width, case.height)
    assert_same_bits(got, lists.words, name)
    return got


@pytest.mark.parametrize("name", sorted(cs.CASES))
def test_lists(renderer, name):
    device_lists(renderer, name)


def test_lists_row_shard(renderer):
    s, _ = restated("cornell")
    assert_same_bits(renderer.camlist(s, 64, 48, 3, 8), cr.camera_lists(s, 64, 48, 3, 8).words)


def render_forced(r, name, scene, spw):
    case = cs.CASES[name]
    ref = oracle_frame(name) if scene is restated(name)[0] else None
    img, ref, st, g = render_pair(r, scene, case.width, case.height, SPP, ref=ref, timing=True, slots_per_wave=spw)
    assert_frame(img, ref)
    counters_equal(g, st, ("segments", "shadow_rays", "draws", "rejected"))
    assert g.schedule == abi.XRT_SCHED_STEP_MERGED
    return g


@pytest.mark.parametrize("spw", [16, 4])
@pytest.mark.parametrize("name", cs.ADVERSARIAL)
def test_frames(renderer, name, spw):
    """the lists first (the frame holds the scene's class, by the device's own lists), then the
    frame with every step launch speculative; the read-back leaves the render as it was"""
    got = device_lists(renderer, name)
    count = cs.check_classes(name, restated(name)[1])
    assert int((got[:, 2] != 0xffffffff).sum()) == count["covered"]
    g = render_forced(renderer, name, restated(name)[0], spw)
    assert g.spec_launches == g.launches[abi.XRT_K_STEP] > 0


def test_65_triangles_no_speculation(renderer):
    """one triangle more than the lists' masks hold: the same schedule without speculative
    launches, and still the oracle's frame"""
    s = cs.tiles_64(extra=True)
    g = render_forced(renderer, "tiles_64", s, 16)
    assert g.spec_launches == 0 and g.launches[abi.XRT_K_STEP] > 0


def test_refusals():
    lib = abi.lib()
    r = HipRenderer(1)
    try:
        out = np.zeros((cs.W * cs.H, 4), np.uint32)
        p = abi.XrtRenderParams(width=cs.W, height=cs.H, spp=1, shard_count=1, max_depth=3)
        assert lib.xrt_test_camlist(r.ctx, C.byref(p), abi.u32ptr(out)) == abi.XRT_ERR_STATE   # nothing uploaded
        assert lib.xrt_test_camlist(r.ctx, None, abi.u32ptr(out)) == abi.XRT_ERR_INVALID
        assert lib.xrt_test_camlist(r.ctx, C.byref(p), None) == abi.XRT_ERR_INVALID
        for scene in (scenes.spheres(cs.W, cs.H, nx=4, nz=2), cs.tiles_64(extra=True)):
            r.upload(scene)
            p = r.params(scene, cs.W, cs.H)
            assert lib.xrt_test_camlist(r.ctx, C.byref(p), abi.u32ptr(out)) == abi.XRT_ERR_STATE
            assert b"1 to 64 triangles" in lib.xrt_last_error(r.ctx)
        assert not out.any()
        s, lists = restated("stacked")   # and the context still serves: a scene it takes
        assert_same_bits(r.camlist(s, cs.W, cs.H), lists.words)
    finally:
        r.close()
