"""The camera lists' emptiness test (tests/camlist_restatement.py, restating k_camlist of
xraytracer_amd/csrc/spec.hip) against the oracle, without a GPU.

The merged schedule finishes a pixel whose camera list is empty without tracing it, as spp
samples of one Scene::intersect call, two draws and radiance +0 each.  That is right only if no
camera ray of such a pixel can hit anything, so here every pixel the restatement calls empty
must show exactly those samples in the oracle's own per-sample record (pyoracle.trace_pixels,
64 spp, every pixel of the frame) — over the Cornell box, the Cornell box far from the origin,
20 random scenes of 1-12 triangles under random cameras, and the silhouette scenes of
tests/test_gpu_elide.py.  Each scene must have pixels of both kinds, or the check is idle.
"""
import numpy as np
import pytest

import pyoracle
from xraytracer_amd import scenes

import camlist_restatement as cr
import elide_scenes as es

SPP = 64


def check(scene, w, h):
    empty = cr.empty_pixels(scene, w, h)
    assert empty.any() and not empty.all(), (int(empty.sum()), empty.size)   # precondition: both kinds
    pix = [(i, j) for i in range(h) for j in range(w)]
    rad, dr, sg = pyoracle.trace_pixels(scene, w, h, SPP, pix)
    e = empty.ravel()
    assert np.all(sg[e] == 1), np.argwhere(np.any(sg != 1, axis=1) & e)[:5]
    assert np.all(dr[e] == 2), np.argwhere(np.any(dr != 2, axis=1) & e)[:5]
    assert np.all(rad[e] == 0.0) and not np.any(np.signbit(rad[e]))
    # the pixels with a sample that hit something: never called empty (the same claim, from the
    # other side) — and the test is not vacuous: most all-miss pixels are called empty
    hit = np.any(sg != 1, axis=1) | np.any(dr != 2, axis=1) | np.any(rad != 0.0, axis=(1, 2))
    assert not np.any(hit & e)
    return empty, hit.reshape(h, w)


def test_cornell():
    empty, hit = check(scenes.cornell(64, 48), 64, 48)
    # the box covers columns 144-656 and rows 48-552 of the 800 x 600 frame: about 46% is background
    assert 0.35 < empty.mean() < 0.46 and hit.mean() > 0.5


def test_cornell_far_from_origin():
    empty, hit = check(es.cornell_shifted(64, 48), 64, 48)
    assert 0.35 < empty.mean() < 0.46 and hit.mean() > 0.5


@pytest.mark.parametrize("seed", range(20))
def test_random_scenes(seed):
    check(es.random_scene(seed), 32, 24)


@pytest.mark.parametrize("name", sorted(es.SILHOUETTES))
def test_silhouettes(name):
    empty, hit = check(es.SILHOUETTES[name](), 32, 24)
    if name == "quarter_pixel":
        i, j = es.QUARTER_PIXEL
        assert hit[i, j] and not empty[i, j]
        assert empty[i - 1, j] and empty[i, j - 1] and empty[i, j + 2]


def test_all_empty_frame():
    """the camera turned away from the Cornell box: every pixel is empty, and the oracle agrees"""
    s = es.cornell_away(64, 32)
    assert cr.empty_pixels(s, 64, 32).all()
    rad, dr, sg = pyoracle.trace_pixels(s, 64, 32, 16, [(i, j) for i in range(0, 32, 5) for j in range(0, 64, 7)])
    assert np.all(sg == 1) and np.all(dr == 2) and np.all(rad == 0.0)


def test_shard_rows():
    """empty_pixels over a row shard marks owned rows only, the same way as over the frame"""
    s = scenes.cornell(64, 48)
    full, part = cr.empty_pixels(s, 64, 48), cr.empty_pixels(s, 64, 48, 3, 8)
    assert np.array_equal(part[3::8], full[3::8]) and part.sum() == full[3::8].sum()
