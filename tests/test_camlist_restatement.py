"""The camera lists (tests/camlist_restatement.py, restating k_camlist of
xraytracer_amd/csrc/spec.hip) against the oracle, without a GPU.

Emptiness (`check_empty`).  The merged schedule finishes a pixel whose camera list is empty
without tracing it, as spp samples of one Scene::intersect call, two draws and radiance +0 each.
That is right only if no camera ray of such a pixel can hit anything, so every pixel the
restatement calls empty must show exactly those samples in the oracle's own per-sample record
(pyoracle.trace_pixels, 64 spp, every pixel of the frame) — over the Cornell box, the Cornell
box far from the origin, 20 random scenes of 1-12 triangles under random cameras, and the
silhouette scenes of tests/test_gpu_elide.py.  Each scene must have pixels of both kinds, or the
check is idle.

The whole list (`check`).  k_step_spec takes a successor sample's first hit from the pixel's list
alone — from its only triangle untested where that one covers the pixel.  So for every pixel of
every scene of tests/camlist_scenes.py, RAYS camera rays through the oracle's own camera
(orc_kat_camera, u and v formed as the oracle's sample loop forms them) must, by the oracle's
Scene::intersect (pyoracle's orc_query), (a) hit nothing but a listed triangle, (b) hit the
covering triangle where the list names one, and (c) miss where the list is empty.  The jitters
are the 6 x 6 grid over {0, 2^-32, 1/4, 1/2, 3/4, the sampler's largest value} and 28 seeded
draws of the sampler's own form per pixel.  Every scene first shows, from the restatement
alone, the pixels it is there for (camlist_scenes.check_classes).
"""
import ctypes as C

import numpy as np
import pytest

import pyoracle
from xraytracer_amd import abi, scenes

import camlist_restatement as cr
import camlist_scenes as cs
import elide_scenes as es

SPP = 64


def check_empty(scene, w, h):
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
    empty, hit = check_empty(scenes.cornell(64, 48), 64, 48)
    # the box covers columns 144-656 and rows 48-552 of the 800 x 600 frame: about 46% is background
    assert 0.35 < empty.mean() < 0.46 and hit.mean() > 0.5


def test_cornell_far_from_origin():
    empty, hit = check_empty(es.cornell_shifted(64, 48), 64, 48)
    assert 0.35 < empty.mean() < 0.46 and hit.mean() > 0.5


@pytest.mark.parametrize("seed", range(20))
def test_random_scenes(seed):
    check_empty(es.random_scene(seed), 32, 24)


@pytest.mark.parametrize("name", sorted(es.SILHOUETTES))
def test_silhouettes(name):
    empty, hit = check_empty(es.SILHOUETTES[name](), 32, 24)
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


# ------------------------------------------------------------------ the whole list ----
F = np.float32
# The largest value the oracle's sampler returns (oracle.c orc_draw: a word that rounds to 2^32
# gives nextafterf(1, 0)), read from its own stream: draw 337 of seed 7302 is such a word.
MAX_DRAW = pyoracle.draws(7302, 1, 337)[0]
GRID = np.array([0.0, 2.0 ** -32, 0.25, 0.5, 0.75, MAX_DRAW], F)
N_RANDOM = 28
RAYS = len(GRID) ** 2 + N_RANDOM


def test_largest_draw():
    assert MAX_DRAW == np.nextafter(F(1.0), F(0.0)) and MAX_DRAW < 1.0
    assert pyoracle.draws(7302, 400).max() == MAX_DRAW and pyoracle.draws(1, 200000).max() <= MAX_DRAW
    assert F(1) / F(4294967296.0) == GRID[1]   # the smallest non-zero draw: the word 1


def jitters(n_pix, seed):
    """[n_pix, RAYS, 2] float32 (r, r'): the grid, then N_RANDOM pairs of draws as orc_draw forms
    them from 32-bit words"""
    gx, gy = np.meshgrid(GRID, GRID, indexing="ij")
    grid = np.stack([gx.ravel(), gy.ravel()], axis=-1)
    words = np.random.default_rng(seed).integers(0, 2 ** 32, (n_pix, N_RANDOM, 2), dtype=np.uint64)
    rnd = words.astype(F) / F(4294967296.0)
    rnd[rnd >= F(1.0)] = MAX_DRAW
    return np.concatenate([np.broadcast_to(grid, (n_pix,) + grid.shape), rnd], axis=1)


def first_hits(scene, w, h, seed=0):
    """[h * w, RAYS] int32: the device's index of the triangle each camera ray hits first by the
    oracle, -1 for a miss.  Rays: Src/renderer.cpp:44-50 through PinholeCamera::sampleRay."""
    lib = pyoracle.lib()
    cam = pyoracle.camera(scene.camera)
    jit = jitters(w * h, seed)
    col = np.tile(np.arange(w, dtype=np.int32), h).astype(F)[:, None]
    row = np.repeat(np.arange(h, dtype=np.int32), w).astype(F)[:, None]
    u = ((col + jit[..., 0]) / F(w)).ravel()
    v = ((row + jit[..., 1]) / F(h)).ravel()
    assert u.dtype == F and v.dtype == F
    n = len(u)
    rays = np.zeros((n, 6), F)
    o, d = (C.c_float * 3)(), (C.c_float * 3)()
    camera, ref = lib.orc_kat_camera, C.byref(cam)
    for q, (uq, vq) in enumerate(zip(u.tolist(), v.tolist())):
        camera(ref, uq, vq, o, d)
        rays[q, :3] = o
        rays[q, 3:] = d
    hits = np.zeros((n, C.sizeof(abi.XrtHit) // 4), np.int32)   # xrt_hit: hit, object, primitive, ...
    assert lib.orc_query(C.byref(scene.desc), n, pyoracle.fp(rays), None, 0,
                         C.cast(hits.ctypes.data, C.POINTER(abi.XrtHit))) == 0
    desc = scene.desc
    first = np.array([desc.objects[k].first for k in range(desc.n_objects)] + [0], np.int32)
    hit, obj, prim = hits[:, 0] != 0, hits[:, 1], hits[:, 2]
    assert np.all((obj >= 0) == hit) and np.all(prim[hit] >= 0)
    return np.where(hit, first[obj] + prim, -1).reshape(w * h, RAYS)


def check(name, lists=None):
    """the three claims of scene `name`'s lists against the oracle, ray by ray; lists: other lists
    than the restatement's, for showing that the proof notices wrong ones"""
    case = cs.CASES[name]
    scene, w, h = case.build(), case.width, case.height
    if lists is None:
        lists = cr.camera_lists(scene, w, h)
        assert np.array_equal(cr.empty_pixels(scene, w, h).ravel(), ~lists.mask.any(axis=1))
        count = cs.check_classes(name, lists)
        print(name, f"{w}x{h}", count, "triangles dropped", int((lists.mask & ~lists.keep).sum()))
    idx = first_hits(scene, w, h)
    assert idx.max() < lists.keep.shape[1]
    hit = idx >= 0
    slot = np.broadcast_to(np.arange(w * h)[:, None], idx.shape)
    listed = np.zeros_like(hit)
    listed[hit] = lists.keep[slot[hit], idx[hit]]
    assert np.all(listed[hit]), ("(a) a ray hits a triangle off the list", name, np.argwhere(hit & ~listed)[:5])
    cov = lists.covering >= 0
    assert np.all(idx[cov] == lists.covering[cov, None]), \
        ("(b) a ray of a covered pixel misses or hits another triangle", name,
         np.argwhere(cov[:, None] & (idx != lists.covering[:, None]))[:5])
    none = ~lists.keep.any(axis=1)
    assert not np.any(hit[none]), ("(c) a ray of an empty pixel hits", name, np.argwhere(hit & none[:, None])[:5])
    return scene, lists, idx


@pytest.mark.parametrize("name", sorted(cs.CASES))
def test_lists(name):
    scene, lists, idx = check(name)
    if name == "coincident":        # the tie: Scene::intersect keeps the first it scans
        assert np.all(idx == 0)
    elif name == "margin_edge":     # every ray of the column hits the triangle that does not cover it
        near, far = cs.margin_pixels()
        assert np.all(idx[near] == 0) and np.all(idx[far] == 1)
    elif name == "stacked":         # the front triangle, second in the scan, wins everywhere
        assert np.all(idx == 1)
    elif name == "tiles_64":
        assert np.any(idx == 31) and np.any(idx == 32) and np.any(idx == 63)


def test_lists_row_shard():
    """camera_lists over a row shard: the owned rows' slots, in slot order"""
    s = scenes.cornell(64, 48)
    full, part = cr.camera_lists(s, 64, 48), cr.camera_lists(s, 64, 48, 3, 8)
    own = (np.arange(3, 48, 8)[:, None] * 64 + np.arange(64)[None, :]).ravel()
    assert len(part.words) == len(own) and np.array_equal(part.words, full.words[own])


def test_wrong_lists_are_noticed():
    """the proof fails on lists a little off: the Cornell lists with a wall taken off one pixel's
    list, with the shortcut pointed at a neighbour triangle, and with an empty pixel's list
    emptied where a ray hits"""
    s = scenes.cornell(64, 48)
    L = cr.camera_lists(s, 64, 48)
    p = int(np.flatnonzero(L.covering >= 0)[0])
    keep = L.keep.copy()
    keep[p, L.covering[p]] = False
    with pytest.raises(AssertionError, match=r"\(a\)"):
        check("cornell", L._replace(keep=keep))
    covering = L.covering.copy()
    covering[p] ^= 1
    with pytest.raises(AssertionError, match=r"\(b\)"):
        check("cornell", L._replace(covering=covering))
    keep = L.keep.copy()
    keep[p] = False
    with pytest.raises(AssertionError, match=r"\((a|c)\)"):
        check("cornell", L._replace(keep=keep, covering=np.full_like(L.covering, -1)))


def test_camlist_entry_refuses_null():
    """xrt_test_camlist checks its arguments before it touches a device"""
    lib = abi.lib()
    assert lib.xrt_test_camlist(None, None, None) == abi.XRT_ERR_INVALID
    p = abi.XrtRenderParams()
    out = np.zeros(4, np.uint32)
    assert lib.xrt_test_camlist(None, C.byref(p), abi.u32ptr(out)) == abi.XRT_ERR_INVALID
