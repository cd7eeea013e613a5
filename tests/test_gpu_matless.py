"""Surfaces without a material (XRT_MAT_NONE, no light) through every schedule, against the oracle.

Object::sampleBxDF returns 0 for such an object and draws nothing (Src/primitive.cpp:39-43): under
GI / Indirect the hit draws two words fewer than a Lambert hit, the throughput becomes 0 and the
next ray has direction (0, 0, 0) — a miss in Mesh::rayTriangleIntersect (det = 0) that still counts
as a Scene::intersect call.  On the device that ray meets the box and plane culls, the pair passes
and the BVH walks with 1 / d = inf.  The scenes are tests/matless_scenes.py's, shown by
tests/test_matless_scenes.py to hold hundreds of such rays and of samples that end on a
material-less hit at the last depth with a successor behind them.

Bar everywhere: the frame bit for bit the oracle's, the sign of a zero included, and segments,
shadow rays, draws and rejects equal to the oracle's.

The speculative kernel (k_step_spec) starts a successor at the stream offsets a sample can have
drawn when it ends over Lamberts and lights (0, 1, 5 words); a last-depth hit on a material-less
object draws 3.  use_step_spec therefore excludes scenes with such objects: the group layouts run
k_step_merged, spec_launches == 0, and the frames are those of spec=False."""
import numpy as np
import pytest

import matless_scenes as ms
from gpu_checks import assert_frame, assert_same_bits, counters_equal, render_pair, renderer  # noqa: F401
from xraytracer_amd import abi

pytestmark = pytest.mark.gpu

TRACED = ("segments", "shadow_rays", "draws", "rejected")
SPEC_DOMAIN = ("cornell_blocks", "cornell_wall")
SCHEDULES = {"auto": None, "step_tri": abi.XRT_SCHED_STEP_TRI, "wavefront": abi.XRT_SCHED_WAVEFRONT}


def check(r, name, expect=None, integrator=None, max_depth=None, shard=None, initial=False, **geo):
    """Render CASES[name] (or the variant the semantic keywords name) with the launch geometry geo
    and compare frame and counters with the oracle; expect: the XRT_SCHED_* it must run, if any.
    Returns (frame, xrt_stats)."""
    _, w, h, spp, _, _ = ms.CASES[name]
    ref = ms.reference(name, integrator=integrator, max_depth=max_depth, shard=shard, initial=initial)
    sem = {}
    if integrator is not None:
        sem["integrator"] = integrator
    if max_depth is not None:
        sem["max_depth"] = max_depth
    if shard is not None:
        sem.update(shard_index=shard[0], shard_count=shard[1])
    if initial:
        sem["initial"] = ms.initial_image(w, h)
    img, want, st, g = render_pair(r, ms.scene(name), w, h, spp, ref=ref, timing=True, **sem, **geo)
    print(f"{name} {sem.keys()} {geo}: schedule {g.schedule} slots_per_wave {g.slots_per_wave} step launches "
          f"{g.launches[abi.XRT_K_STEP]} spec {g.spec_launches} layouts {list(g.layout_launches)} "
          f"counters {[(k, getattr(g, k), st[k]) for k in TRACED]}")
    if expect is not None:
        assert g.schedule == expect, g.schedule
    if geo.get("schedule") == "wavefront":
        assert g.launches[abi.XRT_K_STEP] == 0
    assert_frame(img, want)
    counters_equal(g, st, TRACED)
    return img, g


def check_merged(r, name, **kw):
    """a GI render that runs the merged schedule: none of its launches is speculative"""
    img, g = check(r, name, expect=abi.XRT_SCHED_STEP_MERGED, **kw)
    assert g.spec_launches == 0 and g.launches[abi.XRT_K_STEP] > 0
    return img, g


# ------------------------------------------------------------- the speculative starts' domain ----
@pytest.mark.parametrize("spec", [True, False])
@pytest.mark.parametrize("spw", [16, 8, 4, 0])
@pytest.mark.parametrize("depth", [2, 3, 5])
@pytest.mark.parametrize("name", SPEC_DOMAIN)
def test_group_layouts_and_depths(renderer, name, depth, spw, spec):
    """the layouts in which an all-Lambert scene of this size runs k_step_spec (forced, and the
    library's choice): here they run k_step_merged, with and without XRT_FLAG_NO_SPEC"""
    _, g = check_merged(renderer, name, max_depth=depth, slots_per_wave=spw, spec=spec)
    if spw:
        assert (g.slots_per_wave, g.group_lanes) == (spw, 64 // spw)
    else:
        assert sum(g.layout_launches[2:]) == g.launches[abi.XRT_K_STEP]   # a frame this small: group layouts only


@pytest.mark.parametrize("spw", [16, 4])
@pytest.mark.parametrize("visits", [1, 3, 0])
@pytest.mark.parametrize("name", SPEC_DOMAIN)
def test_samples_and_shadow_rays_cross_launches(renderer, name, visits, spw):
    """1 and 3 visits per launch and the default: samples in progress, pending shadow rays and
    zero-direction rays cross launch boundaries"""
    _, g = check_merged(renderer, name, slots_per_wave=spw, visits_per_launch=visits)
    if visits:
        assert g.visits_per_launch == visits and g.launches[abi.XRT_K_STEP] > 5


@pytest.mark.parametrize("spec", [True, False])
@pytest.mark.parametrize("name", SPEC_DOMAIN)
def test_accumulate(renderer, name, spec):
    check_merged(renderer, name, initial=True, slots_per_wave=16, visits_per_launch=3, spec=spec)


@pytest.mark.parametrize("spec", [True, False])
@pytest.mark.parametrize("name", SPEC_DOMAIN)
def test_row_shard_3_of_8(renderer, name, spec):
    img, _ = check_merged(renderer, name, shard=(3, 8), slots_per_wave=16, spec=spec)
    owned = np.zeros(img.shape[0], bool)
    owned[3::8] = True
    assert np.all(img[~owned] == 0) and img[owned].any()


# ------------------------------------------------------------- the other layouts and schedules ----
@pytest.mark.parametrize("geo", [dict(slots_per_wave=32), dict(slots_per_wave=64), dict(slots_per_wave=16, group=False),
                                 dict(slots_per_wave=32, group=False), dict(interleave=True), dict(interleave=False),
                                 dict(interleave=True, slots_per_wave=64), dict(chunks=True, slots_per_wave=64),
                                 dict(chunks=True, slots_per_wave=64, visits_per_launch=2), dict(overlap=False, slots_per_wave=64),
                                 dict(schedule="step")],
                         ids=lambda g: "-".join(f"{k}={v}" for k, v in g.items()))
@pytest.mark.parametrize("name", SPEC_DOMAIN)
def test_merged_layouts(renderer, name, geo):
    """pair passes over whole and half waves, cooperative passes without group traces, interleaved
    slots, the chunk phase, one launch per round"""
    _, g = check_merged(renderer, name, **geo)
    if "slots_per_wave" in geo:
        assert g.slots_per_wave == geo["slots_per_wave"]
    if "group" in geo:
        assert g.group_lanes == 1


@pytest.mark.parametrize("schedule", ["step_tri", "wavefront"])
@pytest.mark.parametrize("depth", [3, 5])
@pytest.mark.parametrize("name", SPEC_DOMAIN)
def test_per_slot_and_wavefront(renderer, name, depth, schedule):
    """k_step_tri (one cooperative trace per ray kind) and k_shade + k_trace"""
    check(renderer, name, expect=SCHEDULES[schedule], max_depth=depth, schedule=schedule)


# ------------------------------------------------------------- the integrators ----
@pytest.mark.parametrize("schedule", ["auto", "wavefront"])
@pytest.mark.parametrize("integrator,depth", [("indirect", 3), ("indirect", 5), ("direct", 1), ("normal", 1)])
@pytest.mark.parametrize("name", SPEC_DOMAIN)
def test_integrators(renderer, name, integrator, depth, schedule):
    """Indirect (the bounce without light sampling: k_step, k_shade), Direct and Normal (the
    pixel-parallel chains, k_shade)"""
    want = SCHEDULES[schedule]
    if schedule == "auto":
        want = abi.XRT_SCHED_STEP if integrator == "indirect" else abi.XRT_SCHED_PIXEL
    check(renderer, name, expect=want, integrator=integrator, max_depth=depth, schedule=schedule)


@pytest.mark.parametrize("name", SPEC_DOMAIN)
def test_direct_merged(renderer, name):
    """Direct in the merged schedule (XRT_FLAG_NO_PIXEL)"""
    check(renderer, name, expect=abi.XRT_SCHED_STEP_MERGED, integrator="direct", max_depth=1, schedule="step")


# ------------------------------------------------------------- more triangles ----
@pytest.mark.parametrize("schedule", ["auto", "wavefront"])
def test_cornell_mid(renderer, schedule):
    """108 triangles: beyond the camera lists and the group traces, one-level merged (pair passes)"""
    _, g = check(renderer, "cornell_mid", expect=abi.XRT_SCHED_STEP_MERGED if schedule == "auto" else abi.XRT_SCHED_WAVEFRONT,
                 schedule=schedule)
    if schedule == "auto":
        assert g.spec_launches == 0 and g.group_lanes == 1 and g.launches[abi.XRT_K_STEP] > 0


@pytest.mark.parametrize("deep", ["fused", "single", "quad"])
@pytest.mark.parametrize("integrator,depth", [("gi", 3), ("indirect", 4)])
def test_cornell_mesh(renderer, integrator, depth, deep):
    """1,188 triangles, two-level: the merged kernel with the wave's own BVH walk (GI; Indirect
    takes the wavefront there too), and the wavefront schedule with one or four lanes per deep ray"""
    if deep == "fused":
        _, g = check(renderer, "cornell_mesh", integrator=integrator, max_depth=depth, schedule="auto")
        if integrator == "gi":
            assert g.schedule == abi.XRT_SCHED_STEP_BVH and g.launches[abi.XRT_K_DEEP] == 0
    else:
        check(renderer, "cornell_mesh", expect=abi.XRT_SCHED_WAVEFRONT, integrator=integrator, max_depth=depth, deep=deep,
              schedule="wavefront")


@pytest.mark.parametrize("spw", [16, 32, 64])
def test_cornell_mesh_layouts(renderer, spw):
    check(renderer, "cornell_mesh", expect=abi.XRT_SCHED_STEP_BVH, slots_per_wave=spw, visits_per_launch=3)


# ------------------------------------------------------------- material-less by the OBJ loader ----
@pytest.mark.parametrize("spw", [0, 16])
@pytest.mark.parametrize("name", ms.OBJ_CASES)
def test_obj_without_material(renderer, name, spw):
    """an OBJ without materials and an MTL material with `no_surface`: at most 64 triangles, so
    these too would run k_step_spec were they all-Lambert"""
    check_merged(renderer, name, slots_per_wave=spw)


# ------------------------------------------------------------- spheres ----
@pytest.mark.parametrize("schedule", ["auto", "step", "wavefront"])
@pytest.mark.parametrize("integrator", ["direct", "normal", "gi"])
def test_spheres(renderer, integrator, schedule):
    """depth 1 only (matless_scenes: a zero-direction ray on a sphere is undefined in the reference)"""
    want = {"auto": abi.XRT_SCHED_STEP if integrator == "gi" else abi.XRT_SCHED_PIXEL, "step": abi.XRT_SCHED_STEP,
            "wavefront": abi.XRT_SCHED_WAVEFRONT}[schedule]
    check(renderer, "spheres_some", expect=want, integrator=integrator, max_depth=1, schedule=schedule)


# ------------------------------------------------------------- the variance render ----
def test_variance_render(renderer):
    """render_var under XRT_FLAG_VAR_FUSED (the moments build of k_step_merged): the oracle's frame,
    and frame and variance plane the bits of the default (wavefront) variance render"""
    name = "cornell_blocks"
    _, w, h, spp, _, _ = ms.CASES[name]
    ref, st = ms.reference(name)
    renderer.spp = spp
    renderer._uploaded = None
    img, var = renderer.render_var(ms.scene(name), w, h, fused_var=True)
    g = renderer.stats
    assert g.schedule == abi.XRT_SCHED_STEP_MERGED and g.spec_launches == 0
    counters_equal(g, st, TRACED)
    assert_frame(img, ref)
    img0, var0 = renderer.render_var(ms.scene(name), w, h)
    g0 = renderer.stats
    assert g0.schedule == abi.XRT_SCHED_WAVEFRONT
    counters_equal(g0, st, TRACED)
    assert_same_bits(img, img0, "frame")
    assert_same_bits(var, var0, "variance")
    assert np.all(np.isfinite(var)) and var.any()
