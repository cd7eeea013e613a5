"""The trace culls checked on the CPU: for every adversarial ray family (tests/adversarial_rays.py)
over one small scene per trace kernel, no hit of the oracle's may be dropped by the restated culls
(tests/cull_restatement.py) — the hit object's padded box at tlim = t and at FLT_MAX in all slab
forms, the plane cull, the hit triangle's (or sphere's) padded BVH box at tlim = t, each with the
exact float reciprocal and its two neighbours.  The far and shifted families measure where that
stops holding (K_FAIL) and pin the domain the library documents (EXACT_DIAGONALS).

The oracle is the truth throughout, also far from the origin where its hits are geometrically
meaningless: it is the reference's float arithmetic, and that is what the device must return.
"""
from fractions import Fraction

import numpy as np
import pytest

import adversarial_rays as ar
import cull_restatement as cr

F = np.float32
SCENE_NAMES = tuple(ar.SCENES)


def _culls(name, **kw):
    key = ("culls", name, tuple(sorted(kw.items())))
    if key not in ar._cache:
        ar._cache[key] = cr.Culls(ar.scene(name), **kw)
    return ar._cache[key]


def _dropped(culls, b, t=None):
    """{test: rays}: the oracle's hits of batch b that a cull would drop (t: the limit, b.t if None)"""
    c = cr.culled_hits(culls, b.rays, b.object, b.primitive, b.t if t is None else t)
    return {name: np.flatnonzero(m)[:4].tolist() for name, m in c.items() if m.any()}, cr.count_by_structure(c)


# ------------------------------------------------------------------ the restatement's own parts ----
def test_fma32_rounds_once():
    """fma32 against exact rational arithmetic, on slab-like operands and on ties of the double sum"""
    rng = np.random.default_rng(5)
    a = rng.uniform(-600.0, 600.0, 600).astype(F)
    b = np.concatenate([rng.uniform(-4.0, 4.0, 300), 1.0 / rng.uniform(-1e-6, 1e-6, 300)]).astype(F)
    c = -(rng.uniform(-600.0, 600.0, 600).astype(F) * b).astype(F)
    # a * b + c with |c| a float32 half-ulp of the product apart: the double sum is a float32 tie
    a = np.concatenate([a, [F(1.0 + 2.0 ** -23)] * 2, [F(3.0)]])
    b = np.concatenate([b, [F(1.0 + 2.0 ** -23)] * 2, [F(2.0 ** -25)]])
    c = np.concatenate([c, [F(2.0 ** -60), F(-2.0 ** -60), F(1.0)]]).astype(F)
    got = cr.fma32(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo, hi = np.nextafter(g, F(-np.inf)), np.nextafter(g, F(np.inf))
        err = abs(Fraction(float(g)) - exact)
        assert err <= abs(Fraction(float(lo)) - exact) and err <= abs(Fraction(float(hi)) - exact), (x, y, z, g)
        if err == abs(Fraction(float(lo)) - exact) or err == abs(Fraction(float(hi)) - exact):   # a true tie: to even
            assert int(np.asarray(g).view(np.uint32)) % 2 == 0, (x, y, z, g)


def test_pad_formula():
    """Bounds::pad over the Cornell box: 1e-3 of its diagonal + 1e-3; the floor's box reaches that far below y = 0"""
    c, geo = _culls("cornell"), ar.Geometry(ar.scene("cornell"))
    assert abs(float(c.pad_obj) - (1e-3 * geo.diagonal + 1e-3)) < 1e-6 and 0.9 < float(c.pad_obj) < 1.0
    assert float(np.nanmin(c.obj_lo[:, 1])) == float(F(0.0) - c.pad_obj)


def test_scene_kinds():
    """each scene is the kind of trace it is listed for"""
    k = {n: _culls(n) for n in SCENE_NAMES}
    assert k["cornell"].small and len(k["cornell"].v0) <= 64 and (k["cornell"].plane_axis >= 0).sum() >= 5
    assert k["two_level"].two_level and k["two_level"].bvh and not k["two_level"].small
    assert k["mesh"].bvh and not k["mesh"].two_level and not k["mesh"].small and k["mesh"].tri_dropped.any()
    assert k["spheres"].sphere_bvh and k["spheres"].kind == "sphere"
    assert k["smoke"].kind == "mixed" and not (k["smoke"].small or k["smoke"].bvh or k["smoke"].sphere_bvh)
    assert k["synthetic"].small and (k["synthetic"].plane_axis >= 0).sum() == 1
    assert 2.0 < ar.Geometry(ar.scene("synthetic")).diagonal < 2.2


def test_rays_are_finite_and_bounded():
    for name in SCENE_NAMES:
        for fam in ar.FAMILIES:
            r = ar.batch(name, fam).rays
            assert r.dtype == F and np.all(np.isfinite(r)) and np.all(np.any(r[:, 3:] != 0.0, axis=1)), (name, fam)
            assert 200 <= len(r) <= 6000, (name, fam, len(r))


# ------------------------------------------------------------------ no vacuous batches ----
# The reference's own tests make these impossible, and the test says so instead of asserting a count:
#   smoke / limits      BoxMesh::occluded returns true for every ray (Src/primitive.h:266-268), and the
#                       medium's box is an occluder: every occlusion query of the scene answers true
#   synthetic / scaled  the scene's size is about 1: with |d| = 2^-30 every |det| is below FLT_EPSILON, with
#                       |d| = 2^30 every t is: Mesh::rayTriangleIntersect rejects every triangle
IMPOSSIBLE = {("smoke", "limits"): "all occluded", ("synthetic", "scaled"): "all missed"}


@pytest.mark.parametrize("family", ar.FAMILIES)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_batch_not_vacuous(name, family):
    b = ar.batch(name, family)
    answer = b.occluded if family == "limits" else b.object >= 0
    if (name, family) in IMPOSSIBLE:
        assert np.all(answer) if IMPOSSIBLE[(name, family)] == "all occluded" else not np.any(answer)
        return
    assert np.count_nonzero(answer) >= 100 and np.count_nonzero(~answer) >= 100, (int(answer.sum()), len(answer))
    if family != "limits":
        return
    # t is the closest hit of all objects, so nothing can occlude before it: below, at, 0 and -1 are
    # "free" whatever the scene.  The float above t is "occluded" unless the hit object is an area
    # light (Scene::occluded skips those): both answers wherever the scene has one.  FLT_MAX and inf
    # are then "free" only if nothing at all lies behind the light, which a closed scene such as the
    # Cornell box (the ceiling behind its light) does not offer: one answer is all that is possible.
    geo = ar.Geometry(ar.scene(name))
    has_light = any(o[3] >= 0 and o[2] > 0 for o in geo.objects)
    for q, kind in enumerate(ar.LIMIT_KINDS):
        a = b.occluded[b.kinds == q]
        if kind in ("below", "at", "zero", "minus_one"):
            assert not a.any(), kind
        elif kind == "above":
            assert a.any() and (not has_light or not a.all()), (kind, int(a.sum()), len(a))
        else:
            assert a.any(), kind


# ------------------------------------------------------------------ inside any sensible domain ----
@pytest.mark.parametrize("family", ar.FAMILIES)
@pytest.mark.parametrize("name", SCENE_NAMES)
def test_no_hit_culled(name, family):
    b, culls = ar.batch(name, family), _culls(name)
    if family != "limits":
        where, n = _dropped(culls, b)
        assert not where, (n, where, [b.rays[i].tolist() for w in where.values() for i in w[:1]])
        return
    # an occlusion query culls against tmax: where the closest hit is an occluder and t < tmax, that
    # object's tests must keep the ray with the limit tmax
    geo = ar.Geometry(ar.scene(name))
    light = np.array([o[3] >= 0 for o in geo.objects] + [False])
    must = (b.object >= 0) & ~light[b.object] & (b.t < b.tmax)
    assert must.sum() >= 100 or (name, family) in IMPOSSIBLE
    assert np.all(b.occluded[must])
    c = cr.culled_hits(culls, b.rays, np.where(must, b.object, -1), b.primitive, b.tmax)
    assert not any(m.any() for m in c.values()), cr.count_by_structure(c)


# ------------------------------------------------------------------ where exactness ends ----
def _measure():
    """{(structure, family): {k: hits dropped}} over the far batches of every scene and the shifted
    batches of the synthetic scene (with the BVH boxes its triangles would get in a larger scene)"""
    key = "measure"
    if key in ar._cache:
        return ar._cache[key]
    out = {}

    def add(family, k, counts):
        for structure, n in counts.items():
            d = out.setdefault((structure, family), {})
            d[k] = d.get(k, 0) + n

    for k in ar.K_VALUES:
        for name in SCENE_NAMES:
            add("far", k, _dropped(_culls(name), ar.batch(name, "far", k))[1])
        add("far", k, _dropped(_culls("synthetic", force_bvh=True), ar.batch("synthetic", "far", k))[1])
        for direction in ar.SHIFT_DIRECTIONS:
            s, b = ar.shifted_batch(k, direction)
            add("shifted", k, _dropped(cr.Culls(s, force_bvh=True), b)[1])
    out.pop(("sphere_bvh", "shifted"))   # no shifted sphere scene
    ar._cache[key] = out
    return out


def test_k_fail(capsys):
    """the smallest k at which a hit is dropped, per structure and family, is what cull_restatement
    records; EXACT_DIAGONALS lies two octaves below the smallest; nothing is dropped inside it"""
    m = _measure()
    with capsys.disabled():
        print()
        for key in sorted(m):
            print(f"  hits dropped, {key[0]:10s} {key[1]:8s}: " + "  ".join(f"k={k}: {n}" for k, n in m[key].items()))
    k_fail = {key: min((k for k, n in per_k.items() if n), default=None) for key, per_k in m.items()}
    assert k_fail == cr.K_FAIL
    assert cr.EXACT_DIAGONALS == 2.0 ** (min(k_fail.values()) - 2)
    assert cr.EXACT_DIAGONALS_TRI == 2.0 ** (min(v for (s, _), v in k_fail.items() if s != "sphere_bvh") - 2)
    for (structure, family), per_k in m.items():
        limit = cr.EXACT_DIAGONALS if structure == "sphere_bvh" else cr.EXACT_DIAGONALS_TRI
        assert all(n == 0 for k, n in per_k.items() if 2.0 ** k <= limit), (structure, family, per_k)


def test_header_states_the_measured_domain():
    """include/xrt.h's XRT_EXACT_DIAGONALS / XRT_EXACT_DIAGONALS_TRI are the measured numbers"""
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "xrt.h")) as f:
        text = f.read()
    macros = dict(re.findall(r"^#define (XRT_EXACT_DIAGONALS\w*) ([0-9.]+)f$", text, re.M))
    assert {k: float(v) for k, v in macros.items()} == {"XRT_EXACT_DIAGONALS": cr.EXACT_DIAGONALS,
                                                        "XRT_EXACT_DIAGONALS_TRI": cr.EXACT_DIAGONALS_TRI}


@pytest.mark.parametrize("name", SCENE_NAMES)
def test_far_batches_in_domain(name):
    """inside the scene's domain the far batches hold both answers and lose no hit"""
    culls = _culls(name)
    ks = [k for k in ar.K_VALUES if 2.0 ** k <= cr.exact_diagonals(culls.kind)]
    assert ks and ks[0] == 0
    for k in ks:
        b = ar.batch(name, "far", k)
        hits = np.count_nonzero(b.object >= 0)
        assert hits >= 100 and len(b.rays) - hits >= 100, (k, hits, len(b.rays))
        assert 200 <= len(b.rays) <= 6000
        where, n = _dropped(culls, b)
        assert not where, (k, n, where)


def test_shifted_batches_in_domain():
    for direction in ar.SHIFT_DIRECTIONS:
        for k in [k for k in ar.K_VALUES if 2.0 ** k <= cr.EXACT_DIAGONALS_TRI]:
            s, b = ar.shifted_batch(k, direction)
            hits = np.count_nonzero(b.object >= 0)
            assert hits >= 100 and len(b.rays) - hits >= 100, (direction, k, hits, len(b.rays))
            where, n = _dropped(cr.Culls(s, force_bvh=True), b)
            assert not where, (direction, k, n, where)
