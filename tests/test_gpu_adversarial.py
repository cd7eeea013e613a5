"""The trace kernels against the oracle on the adversarial ray families (tests/adversarial_rays.py),
inside the domain tests/test_adversarial_rays.py has measured on the CPU (cull_restatement.
EXACT_DIAGONALS): grazing rays, rays in a wall's plane, axis-parallel rays on box faces, far
origins, a scene far from the world origin, scaled directions, shadow limits around the hit.

xrt_query reaches the wavefront trace kernels, one small scene per kernel: closest-hit records
equal in every field, bit for bit, and occlusion flags equal.  The fused, merged, speculative,
pixel-parallel, Whitted and guide-buffer kernels trace through LDS scene code of their own and are
reachable only through a camera: they render the Cornell box and the two-level sphere-mesh scene
through a camera moved back to 1 and to EXACT_DIAGONALS_TRI scene diagonals (the sphere scene: to
EXACT_DIAGONALS), with the field of view shrunk so that the framing stays — the silhouettes stay in
the image, so the culls are met at their edges — against the oracle's frame and counters.  Beyond
the domain nothing is asserted.
"""
import functools

import numpy as np
import pytest

import adversarial_rays as ar
import aov_restatement
import cull_restatement as cr
import pyoracle
import whitted_bvh_scenes as wb
import whitted_restatement as wr
import whitted_scenes as ws
from gpu_checks import assert_frame, assert_same_bits, counters_equal, render_pair, renderer  # noqa: F401
from test_gpu_query import FIELDS
from xraytracer_amd import abi, scenes

pytestmark = pytest.mark.gpu

# the words of an xrt_hit by field, in test_gpu_query's order of comparison
WORD_FIELD = [name for name, ctype in abi.XrtHit._fields_ for _ in range(max(1, getattr(ctype, "_length_", 1)))]
assert tuple(dict.fromkeys(WORD_FIELD)) == FIELDS


def check_queries(r, scene, b, what):
    """batch b through xrt_query: the records of the closest-hit query (an occlusion batch: the
    flags) equal the oracle's; and the same rays as shadow rays"""
    if b.tmax is None:
        got = ar.hit_table(r.query(scene, b.rays))
        bad = np.flatnonzero(np.any(got != b.table, axis=1))
        first = [(int(i), b.rays[i].tolist(), sorted({WORD_FIELD[w] for w in np.flatnonzero(got[i] != b.table[i])}))
                 for i in bad[:3]]
        assert not len(bad), (what, f"{len(bad)} of {len(got)} records differ", first)
    tmax = b.shadow_tmax if b.tmax is None else b.tmax
    occ = np.array([h.hit for h in r.query(scene, b.rays, tmax=tmax, occluded=True)], bool)
    bad = np.flatnonzero(occ != b.occluded)
    assert not len(bad), (what, f"{len(bad)} of {len(occ)} flags differ", [(int(i), b.rays[i].tolist(), float(tmax[i])) for i in bad[:3]])


def test_scene_kinds():
    """each scene reaches the trace kernel it is listed for (what upload_scene_one builds, restated)"""
    k = {n: cr.Culls(ar.scene(n)) for n in ar.SCENES}
    assert k["cornell"].small and k["synthetic"].small
    assert k["two_level"].two_level and k["mesh"].bvh and not k["mesh"].two_level
    assert k["spheres"].sphere_bvh and k["smoke"].kind == "mixed"


@pytest.mark.parametrize("family", ar.FAMILIES)
@pytest.mark.parametrize("name", tuple(ar.SCENES))
def test_query_family(renderer, name, family):
    check_queries(renderer, ar.scene(name), ar.batch(name, family), (name, family))


@pytest.mark.parametrize("name", tuple(ar.SCENES))
def test_query_far_origins(renderer, name):
    limit = cr.exact_diagonals(cr.Culls(ar.scene(name)).kind)
    ks = [k for k in ar.K_VALUES if 2.0 ** k <= limit]
    assert ks
    for k in ks:
        check_queries(renderer, ar.scene(name), ar.batch(name, "far", k), (name, "far", k))


@pytest.mark.parametrize("direction", tuple(ar.SHIFT_DIRECTIONS))
def test_query_shifted_scene(renderer, direction):
    for k in [k for k in ar.K_VALUES if 2.0 ** k <= cr.EXACT_DIAGONALS_TRI]:
        s, b = ar.shifted_batch(k, direction)
        assert cr.Culls(s).small
        check_queries(renderer, s, b, ("shifted", direction, k))


# ------------------------------------------------------------------ far cameras ----
W, H = 32, 24
DISTANCES = (1.0, cr.EXACT_DIAGONALS_TRI)    # both scenes are triangle scenes
TRACED = ("segments", "shadow_rays", "draws", "rejected")


@functools.lru_cache(maxsize=None)
def camera_scene(name, diagonals):
    """"cornell", "two_level", "whitted" (the two-level scene with a point light) or "spheres" seen
    from `diagonals` scene diagonals"""
    s = {"cornell": lambda: scenes.cornell(W, H), "two_level": lambda: scenes.cornell_spheremesh(W, H, n_theta=40, n_phi=40),
         "whitted": lambda: wb.pinned(W, H), "spheres": lambda: scenes.spheres(W, H, 32, 18)}[name]()
    s.camera = ar.far_camera(s, diagonals)
    return s


@functools.lru_cache(maxsize=None)
def guide(name, diagonals):
    """the restated guide planes of the view at 2 samples; the object's silhouette lies inside the
    image: hit and miss pixels both, and none but misses on the image's border (the sphere scene: many
    silhouettes, of which the rows of spheres run out of the image — hit and miss pixels both)"""
    planes, cnt, _ = aov_restatement.render(camera_scene(name, diagonals), W, H, 2)
    alpha = planes["alpha"]
    border = np.concatenate([alpha[0], alpha[-1], alpha[:, 0], alpha[:, -1]])
    assert name == "spheres" or not border.any()
    assert np.count_nonzero(alpha == 1.0) >= 100 and np.count_nonzero(alpha == 0.0) >= 100
    return planes, cnt


@functools.lru_cache(maxsize=None)
def oracle_frame(name, diagonals, spp, integrator):
    return pyoracle.render(camera_scene(name, diagonals), W, H, spp, integrator=integrator)


def check_render(r, name, diagonals, spp, expect, integrator="gi", **kw):
    guide(name, diagonals)
    s = camera_scene(name, diagonals)
    img, ref, st, g = render_pair(r, s, W, H, spp, ref=oracle_frame(name, diagonals, spp, integrator),
                                  integrator=integrator, **kw)
    assert g.schedule == expect, (g.schedule, expect)
    counters_equal(g, st, TRACED)
    assert_frame(img, ref)
    return g


@pytest.mark.parametrize("diagonals", DISTANCES)
def test_far_camera_cornell_gi(renderer, diagonals):
    g = check_render(renderer, "cornell", diagonals, 3, abi.XRT_SCHED_STEP_MERGED, slots_per_wave=16)
    assert g.slots_per_wave == 16 and g.spec_launches > 0                 # speculative
    g = check_render(renderer, "cornell", diagonals, 3, abi.XRT_SCHED_STEP_MERGED, slots_per_wave=64, spec=False)
    assert g.slots_per_wave == 64 and g.spec_launches == 0
    check_render(renderer, "cornell", diagonals, 3, abi.XRT_SCHED_STEP_TRI, schedule="step_tri")
    check_render(renderer, "cornell", diagonals, 3, abi.XRT_SCHED_STEP_MERGED, schedule="step")
    check_render(renderer, "cornell", diagonals, 3, abi.XRT_SCHED_WAVEFRONT, schedule="wavefront")


@pytest.mark.parametrize("integrator", ["direct", "normal"])
@pytest.mark.parametrize("diagonals", DISTANCES)
def test_far_camera_cornell_one_hit(renderer, diagonals, integrator):
    check_render(renderer, "cornell", diagonals, 4, abi.XRT_SCHED_PIXEL, integrator=integrator)
    # per-slot: Direct in the merged kernel, Normal (no merged or cooperative form) in k_step
    per_slot = abi.XRT_SCHED_STEP_MERGED if integrator == "direct" else abi.XRT_SCHED_STEP
    check_render(renderer, "cornell", diagonals, 4, per_slot, integrator=integrator, schedule="step")


def test_far_camera_spheres(renderer):
    """the sphere BVH and the pixel-parallel schedule's padded balls (pixel.hip), which no query
    reaches, from the edge of the domain of a sphere scene"""
    d = cr.EXACT_DIAGONALS
    check_render(renderer, "spheres", d, 4, abi.XRT_SCHED_PIXEL, integrator="direct")
    check_render(renderer, "spheres", d, 4, abi.XRT_SCHED_STEP, integrator="direct", schedule="step")
    check_render(renderer, "spheres", d, 4, abi.XRT_SCHED_WAVEFRONT, integrator="direct", schedule="wavefront")
    ref, cnt = guide("spheres", d)
    renderer.spp = 2
    renderer._uploaded = None
    got = renderer.render_aov(camera_scene("spheres", d), W, H)
    for k in aov_restatement.PLANES:
        assert_same_bits(got[k], ref[k], k)


@pytest.mark.parametrize("diagonals", DISTANCES)
def test_far_camera_two_level_gi(renderer, diagonals):
    for deep in ("single", "quad"):
        check_render(renderer, "two_level", diagonals, 2, abi.XRT_SCHED_STEP_BVH, deep=deep)
        check_render(renderer, "two_level", diagonals, 2, abi.XRT_SCHED_WAVEFRONT, schedule="wavefront", deep=deep)


@pytest.mark.parametrize("diagonals", DISTANCES)
def test_far_camera_two_level_whitted(renderer, diagonals):
    guide("whitted", diagonals)
    s = camera_scene("whitted", diagonals)
    ref, cnt, _ = wr.render(s, W, H, 2, max_depth=3)
    renderer.spp = 2
    renderer._uploaded = None
    img = renderer.render(s, W, H, max_depth=3, whitted_bvh=True)
    st = renderer.stats
    assert st.schedule == abi.XRT_SCHED_WHITTED_BVH
    assert {k: int(getattr(st, k)) for k in ws.COUNTERS} == {k: int(cnt[k]) for k in ws.COUNTERS}
    assert_frame(img, ref)


@pytest.mark.parametrize("name", ["cornell", "two_level"])
@pytest.mark.parametrize("diagonals", DISTANCES)
def test_far_camera_guide_buffers(renderer, diagonals, name):
    ref, cnt = guide(name, diagonals)
    renderer.spp = 2
    renderer._uploaded = None
    got = renderer.render_aov(camera_scene(name, diagonals), W, H)
    st = renderer.stats
    assert {k: int(getattr(st, k)) for k in aov_restatement.COUNTERS} == {k: int(cnt[k]) for k in aov_restatement.COUNTERS}
    for k in aov_restatement.PLANES:
        assert_same_bits(got[k], ref[k], k)
