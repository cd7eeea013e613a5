"""Camera rays of covered pixels, not traced (XRT_CAM_COVER: k_camlist writes a pixel's covering
triangle into the slot's state word where it retires the empty pixels, and k_step_merged gives a
depth-0 extension ray of such a slot that triangle instead of a trace) against the oracle.

The covering claim itself — every camera ray of the pixel hits that triangle first — is proven by
tests/test_camlist_restatement.py and the device's lists by tests/test_gpu_camlist.py; here the
frames that the shortcut renders.  Bar: framebuffer bit for bit and segments, shadow rays, draws and
rejects equal to the oracle's, on every scene of tests/camlist_scenes.py at its own size, in full
waves (64 slots per wave) and in the layout the library picks, after the device's own lists
(HipRenderer.camlist, shown equal to the restatement's) have shown that the frame holds covered and
uncovered pixels.  Five scenes hold no covered pixel by the restatement (NO_COVER: the coincident
and the stacked triangles, where a tie or a near tie must keep the shortcut off, and three random
scenes); there the lists must say so, and the frame shows that nothing was shortcut.  Then the
Cornell box with depth-0 rays crossing launches (1, 2, 3 visits per launch), with and without
speculative launches, as a row shard, and added to an image that holds -0.0."""
import numpy as np
import pytest

import pyoracle
from gpu_checks import assert_frame, assert_same_bits, counters_equal, render_pair, renderer  # noqa: F401
from xraytracer_amd import abi

import camlist_scenes as cs
from test_gpu_camlist import SPP, device_lists, oracle_frame, restated

pytestmark = pytest.mark.gpu

TRACED = ("segments", "shadow_rays", "draws", "rejected")
NO_COVER = {"coincident", "stacked", "random_00", "random_03", "random_15"}


def covered_pixels(r, name):
    """[slots] bool from the device's lists: has the pixel a covering triangle?  Both kinds are
    there (NO_COVER: none is covered)."""
    got = device_lists(r, name)
    cov = got[:, 2] != 0xffffffff
    assert np.array_equal(cov, restated(name)[1].covering >= 0)
    assert (~cov & ((got[:, 0] | got[:, 1]) != 0)).any(), name   # uncovered pixels with triangles to trace
    assert cov.any() != (name in NO_COVER), (name, int(cov.sum()))
    return cov


def render_cover(r, name, ref=None, **kw):
    case = cs.CASES[name]
    ref = oracle_frame(name) if ref is None else ref
    img, ref, st, g = render_pair(r, restated(name)[0], case.width, case.height, SPP, ref=ref, timing=True, **kw)
    assert g.schedule == abi.XRT_SCHED_STEP_MERGED and g.launches[abi.XRT_K_SEED] == 2   # k_camlist ran beside k_seed
    counters_equal(g, st, TRACED)
    return img, ref, g


@pytest.mark.parametrize("spw", [64, 0])
@pytest.mark.parametrize("name", sorted(cs.CASES))
def test_scenes(renderer, name, spw):
    covered_pixels(renderer, name)
    img, ref, g = render_cover(renderer, name, slots_per_wave=spw)
    assert_frame(img, ref)
    if spw:
        assert (g.slots_per_wave, g.group_lanes) == (64, 1)


@pytest.mark.parametrize("spw", [64, 32])
@pytest.mark.parametrize("visits", [1, 2, 3])
def test_depth0_rays_cross_launches(renderer, visits, spw):
    """with one visit per launch every camera ray is stored at depth 0 without ST_REGEN and traced —
    or not — by the next launch, which must still find the covering triangle in the state word;
    32 slots per wave: the merged kernel's group-trace build"""
    covered_pixels(renderer, "cornell")
    img, ref, g = render_cover(renderer, "cornell", visits_per_launch=visits, slots_per_wave=spw)
    assert_frame(img, ref)
    assert g.visits_per_launch == visits and g.slots_per_wave == spw and g.spec_launches == 0


@pytest.mark.parametrize("spec", [False, True])
@pytest.mark.parametrize("name", ["cornell", "emissive_cover", "tiles_64"])
def test_with_and_without_speculation(renderer, name, spec):
    """16 slots per wave: k_step_spec, which drops the covering bits when it stores a slot, or the
    merged kernel's group-trace build, which reads them"""
    covered_pixels(renderer, name)
    img, ref, g = render_cover(renderer, name, slots_per_wave=16, visits_per_launch=3, spec=spec)
    assert_frame(img, ref)
    assert g.spec_launches == (g.launches[abi.XRT_K_STEP] if spec else 0)


def test_row_shard(renderer):
    """shard 3 of 8: the covering triangles are indexed by slot, as the lists are"""
    s, _ = restated("cornell")
    w, h = 64, 48
    got = renderer.camlist(s, w, h, 3, 8)
    cov = got[:, 2] != 0xffffffff
    assert cov.any() and (~cov & ((got[:, 0] | got[:, 1]) != 0)).any()
    ref = pyoracle.render(s, w, h, SPP, shard_index=3, shard_count=8)
    img, ref, st, g = render_pair(renderer, s, w, h, SPP, ref=ref, slots_per_wave=64, shard_index=3, shard_count=8)
    owned = np.zeros(h, bool)
    owned[3::8] = True
    assert_frame(img[owned], ref[owned])
    assert np.all(img[~owned] == 0) and g.path_slots == owned.sum() * w
    counters_equal(g, st, TRACED)


def test_accumulates_over_negative_zero(renderer):
    """added to an image whose entries include -0.0, in covered pixels too"""
    case = cs.CASES["cornell"]
    w, h = case.width, case.height
    cov = covered_pixels(renderer, "cornell").reshape(h, w)
    rng = np.random.default_rng(17)
    init = rng.uniform(0.0, 2.0, (h, w, 3)).astype(np.float32)
    init[rng.random((h, w, 3)) < 0.2] = -0.0
    assert np.signbit(init[cov]).sum() > 100 and np.signbit(init[~cov]).sum() > 100
    ref = pyoracle.render(restated("cornell")[0], w, h, SPP, initial=init)
    img, ref, g = render_cover(renderer, "cornell", ref=ref, initial=init, slots_per_wave=64)
    assert_frame(img, ref)
