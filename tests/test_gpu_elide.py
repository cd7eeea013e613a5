"""Pixels no camera ray can hit, finished before the path loop (k_camlist's `retire`,
xraytracer_amd/csrc/spec.hip) against the oracle.

In the merged schedule a GIIntegrator pixel whose camera list is empty gets, right after the
seeding refill, the state its spp one-segment samples would have left (Src/renderer.cpp:29-81,
Src/integrator.h:205-287: two draws, one Scene::intersect, radiance +0 each) and is never
traced.  Bar: framebuffers bit for bit — the sign of a zero included — and segments, shadow
rays, draws and rejects equal to the oracle's.  Cases: a frame of empty pixels only (over an
image that holds -0.0), the Cornell box in the 64-slot, the speculative 16- and 4-slot layouts
and without speculation, silhouettes where a wrong "empty" would show (each first shown, from
the oracle, to have hitting samples where it matters), and a row shard added in place.
tests/test_camlist_restatement.py checks the emptiness test itself without a GPU.
"""
import numpy as np
import pytest

import pyoracle
from gpu_checks import assert_frame, assert_same_bits, counters_equal, render_pair, renderer  # noqa: F401
from xraytracer_amd import abi, scenes

import elide_scenes as es

pytestmark = pytest.mark.gpu


def render_elide(r, scene, w, h, spp, ref=None, **kw):
    """the device's frame and the oracle's (`ref`: an (image, stats) pair computed before), the
    counters compared; a camera-list launch beside k_seed shows that the pixels were tested"""
    img, ref, st, g = render_pair(r, scene, w, h, spp, ref=ref, timing=True, **kw)
    assert g.schedule == abi.XRT_SCHED_STEP_MERGED and g.launches[abi.XRT_K_SEED] == 2
    counters_equal(g, st, ("segments", "shadow_rays", "draws", "rejected"))
    return img, ref, st, g


def hits(scene, w, h, spp):
    """[h, w] bool from the oracle's per-sample record: does a sample of the pixel hit anything?"""
    rad, dr, sg = pyoracle.trace_pixels(scene, w, h, spp, [(i, j) for i in range(h) for j in range(w)])
    return (np.any(sg != 1, axis=1) | np.any(dr != 2, axis=1) | np.any(rad != 0.0, axis=(1, 2))).reshape(h, w)


def test_all_empty_frame(renderer):
    """The camera turned away from the Cornell box, 700 spp: no slot is traced, so none twists
    its ring again (1,400 draws would, twice), one step launch drops them all, and the image's
    -0.0 entries become +0."""
    w, h, spp = 64, 32, 700
    s = es.cornell_away(w, h)
    rng = np.random.default_rng(11)
    init = rng.uniform(0.0, 3.0, (h, w, 3)).astype(np.float32)
    init[rng.random((h, w, 3)) < 0.1] = -0.0
    assert np.signbit(init).sum() > 100
    img, ref, st, g = render_elide(renderer, s, w, h, spp, initial=init)
    assert_frame(img, ref)
    assert not np.any(np.signbit(img))
    assert g.rng_twists == g.path_slots == w * h
    assert g.launches[abi.XRT_K_STEP] < -(-spp // g.visits_per_launch)
    assert g.segments == g.samples == w * h * spp and g.draws == 2 * g.samples


@pytest.fixture(scope="module")
def cornell_ref():
    s = scenes.cornell(64, 48)
    return s, pyoracle.render(s, 64, 48, 40)


@pytest.mark.parametrize("spw,spec", [(64, True), (16, True), (4, True), (16, False)])
def test_cornell_layouts(renderer, cornell_ref, spw, spec):
    """40 spp at 3 visits per launch: the retired slots sit in the first launch's list beside
    slots that run for a hundred launches more, in every kernel that can be the first."""
    s, ref = cornell_ref
    img, ref, st, g = render_elide(renderer, s, 64, 48, 40, ref=ref, slots_per_wave=spw, visits_per_launch=3, spec=spec)
    assert_frame(img, ref)
    assert g.visits_per_launch == 3 and g.slots_per_wave == spw
    if spw == 64:
        assert g.spec_launches == 0
    else:
        assert g.spec_launches == (g.launches[abi.XRT_K_STEP] if spec else 0)


def check_silhouette(name, hit):
    h, w = hit.shape
    if name == "quarter_pixel":   # the speck's pixel, alone in the upper frame
        i, j = es.QUARTER_PIXEL
        assert hit[i, j] and hit[:16].sum() == 1
    elif name == "sliver":        # the strip is hit in every row above the floor
        assert np.all(hit[:16].sum(axis=1) >= 1) and hit[:16].sum() < 3 * 16 + 8
    elif name == "edge_on":       # the blade shows in one row only, across most of it
        rows = np.flatnonzero(hit[6:].sum(axis=1)) + 6
        assert list(rows) == [11] and hit[11].sum() >= 20
    elif name == "near_wall":     # the wall fills the left half; beside it, pixels nothing fills
        assert np.all(hit[:, :w // 2]) and not np.any(hit[:, w // 2 + 1:w // 2 + 8])
    else:
        raise KeyError(name)


@pytest.mark.parametrize("name", sorted(es.SILHOUETTES))
def test_silhouettes(renderer, name):
    w, h, spp = 32, 24, 40
    s = es.SILHOUETTES[name]()
    check_silhouette(name, hits(s, w, h, spp))
    img, ref, st, g = render_elide(renderer, s, w, h, spp)
    assert_frame(img, ref)


def test_cornell_far_from_origin(renderer):
    """The box and its camera translated by 1e4: the vertices sit on a 1e-3 grid, the margins
    of the emptiness test are relative to the vectors from the eye."""
    w, h, spp = 64, 48, 16
    s = es.cornell_shifted(w, h)
    hit = hits(s, w, h, spp)
    edge = hit & ~(np.roll(hit, 1, 0) & np.roll(hit, -1, 0) & np.roll(hit, 1, 1) & np.roll(hit, -1, 1))
    assert hit.mean() > 0.5 and (~hit).mean() > 0.3 and edge.sum() > 100   # a silhouette all round the box
    img, ref, st, g = render_elide(renderer, s, w, h, spp)
    assert_frame(img, ref)


def test_row_shard_accumulates(renderer):
    """Rows y % 8 == 3 of the Cornell frame added to an image in place: owned rows as the
    oracle's, the others untouched."""
    w, h, spp = 64, 48, 24
    s = scenes.cornell(w, h)
    init = np.random.default_rng(3).uniform(0.0, 2.0, (h, w, 3)).astype(np.float32)
    init[5, 7] = -0.0      # not owned
    init[3, 0] = -0.0      # owned, empty
    img, ref, st, g = render_elide(renderer, s, w, h, spp, initial=init, shard_index=3, shard_count=8)
    owned = np.zeros(h, bool)
    owned[3::8] = True
    assert_frame(img[owned], ref[owned])
    assert_same_bits(img[~owned], init[~owned])
    assert g.path_slots == owned.sum() * w
