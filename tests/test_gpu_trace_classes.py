"""The merged trace's class streams (merged_trace, xraytracer_amd/csrc/merged.h) against the
oracle: objects of equal triangle count rank their rays into one LDS stream and share its pair
passes, a ranked ray carrying its object's first triangle.  Bar for every case: framebuffer bit for
bit and the path counters equal to the oracle's, in full waves (64 slots per wave, the pair-pass
layout).  tests/test_step_classes.py checks the host grouping without a GPU.

Cases: the Cornell box (classes of 2, 6 and 10 triangles) under GIIntegrator and, with a second
light, under DirectIntegrator in the merged schedule (three rays per lane); a stack of quads whose
one class overflows the ranked-ray buffer, shown from the boxes first — under DirectIntegrator, and
under GIIntegrator with no pixel covered, so that every camera ray is ranked; two coincident objects of one
class, where the tie goes to the lower triangle index; single-triangle objects beside a 3-triangle
one; and the small two-level scene of tests/test_gpu_configs.py, whose keys carry original
indices."""
import numpy as np
import pytest

import pyoracle
from gpu_checks import assert_frame, assert_same_bits, counters_equal, render_pair, renderer  # noqa: F401
from xraytracer_amd import abi, scenes

import camlist_restatement as cr
import elide_scenes as es
from test_gpu_configs import C4_TWIST_SPP, c4_twist_reference

pytestmark = pytest.mark.gpu


def render_full_waves(r, scene, w, h, spp, ref=None, sched=abi.XRT_SCHED_STEP_MERGED, **kw):
    """the frame and counters against the oracle's at 64 slots per wave, pair passes"""
    img, ref, st, g = render_pair(r, scene, w, h, spp, ref=ref, slots_per_wave=64, **kw)
    assert g.schedule == sched and (g.slots_per_wave, g.group_lanes) == (64, 1)
    assert_frame(img, ref)
    counters_equal(g, st)
    return img, g


def object_counts(scene):
    d = scene.desc
    return [d.objects[k].count for k in range(d.n_objects)]


def test_cornell_gi(renderer):
    s = scenes.cornell(96, 72)
    assert sorted(set(object_counts(s))) == [2, 6, 10]
    render_full_waves(renderer, s, 96, 72, 8)


def test_cornell_direct_two_lights(renderer):
    """DirectIntegrator outside the pixel schedule: one extension and two shadow rays per lane"""
    s = scenes.SceneBundle()
    s.load_obj(scenes.CORNELL_OBJ)
    s.add_quad_light("QuadLight", (343.0, 548.0, 227.0), (343.0, 548.0, 332.0), (213.0, 548.0, 227.0), (25.0, 25.0, 25.0))
    s.add_quad_light("SideLight", (1.0, 200.0, 200.0), (1.0, 300.0, 200.0), (1.0, 200.0, 300.0), (9.0, 12.0, 15.0))   # faces the room
    s.flatten()
    s.camera = scenes.pinhole(scenes.CORNELL_C2W, 60.0, 96, 72)
    assert s.desc.n_lights == 2
    img, g = render_full_waves(renderer, s, 96, 72, 8, integrator="direct", schedule="step")
    one = pyoracle.render(scenes.cornell(96, 72), 96, 72, 8, integrator="direct")[1]   # the same frame, first light only
    assert g.segments == one["segments"] and g.shadow_rays > one["shadow_rays"]   # the second light is sampled too


# ------------------------------------------------------------------ overflow ----
STACK_W, STACK_H, STACK_N = 32, 16, 6


def stack_quads():
    """STACK_N quads across the whole frame at depths 5 .. 10, each bent out of every axis plane"""
    w, h = STACK_W, STACK_H
    quads = []
    for k in range(STACK_N):
        z = 5.0 + k
        a, b = es.at(w, h, -8.0, -8.0, z + 0.05), es.at(w, h, w + 8.0, -8.0, z - 0.03)
        c, d = es.at(w, h, w + 8.0, h + 8.0, z + 0.02), es.at(w, h, -8.0, h + 8.0, z - 0.04)
        quads.append(np.array([(a, c, b), (a, d, c)], np.float64))   # facing the eye
    return quads


def stack_scene(twice=False):
    """twice: the front quad a second time, as an object of its own with the same vertices — then
    no triangle is alone in any pixel's camera list, so no pixel has a covering triangle"""
    s = es.eye_scene(STACK_W, STACK_H)
    quads = stack_quads()
    for k, q in enumerate(quads):
        s.add_mesh(f"quad_{k}", q, (0.3 + 0.1 * k, 0.8 - 0.1 * k, 0.5))
    if twice:
        s.add_mesh("quad_0_again", quads[0], (0.2, 0.3, 0.9))
    s.add_quad_light("lamp", (-2.0, 3.0, -1.0), (-2.0, 3.0, -4.0), (2.0, 3.0, -1.0), (20.0, 20.0, 20.0))   # faces down
    s.flatten()
    return s


def every_camera_ray_enters_every_box():
    """the directions from the eye that meet a convex box form a convex cone, and the four corner
    directions of every pixel lie in it, so every jittered ray between them does"""
    w, h = STACK_W, STACK_H
    xs, ys = np.meshgrid(np.arange(w + 1.0), np.arange(h + 1.0))
    dirs = np.stack(es.at(w, h, xs, ys, 1.0 + 0 * xs), axis=-1).reshape(-1, 3)   # pixel corners, from the eye at 0
    for q in stack_quads():
        lo, hi = q.reshape(-1, 3).min(axis=0), q.reshape(-1, 3).max(axis=0)   # inside the device's padded box
        with np.errstate(divide="ignore"):
            t0, t1 = lo / dirs, hi / dirs
        tn, tf = np.minimum(t0, t1).max(axis=1), np.maximum(t0, t1).min(axis=1)
        assert np.all(tn <= tf) and np.all(tf > 0)


def test_stack_overflows_the_ranked_buffer_direct(renderer):
    """DirectIntegrator in the merged schedule with one light: 2 * 64 ranked rays at most, and no
    covering shortcut (it is compiled for GIIntegrator only), so every camera ray is traced.  Every
    camera ray of the frame enters the box of every quad, and within the quads' class no object
    culls another, so a wave's 64 camera rays rank 64 * STACK_N records: more than the buffer
    holds, whatever the order of the objects."""
    s = stack_scene()
    assert object_counts(s).count(2) >= STACK_N >= 5 and s.desc.n_lights == 1
    every_camera_ray_enters_every_box()
    assert 64 * STACK_N > (1 + s.desc.n_lights) * 64
    render_full_waves(renderer, s, STACK_W, STACK_H, 6, integrator="direct", schedule="step")


def test_stack_overflows_the_ranked_buffer_gi(renderer):
    """The same under GIIntegrator, where a covered pixel's camera rays are not traced: with the
    front quad there twice no pixel is covered — shown from the restated camera lists, which the
    device's are required to equal — so again every camera ray of every wave is ranked once per
    quad, 64 * (STACK_N + 1) records against 2 * 64."""
    w, h = STACK_W, STACK_H
    s = stack_scene(twice=True)
    assert object_counts(s).count(2) >= STACK_N + 1 and s.desc.n_lights == 1
    every_camera_ray_enters_every_box()
    lists = cr.camera_lists(s, w, h)
    assert np.all(lists.covering == -1) and np.all(lists.keep.sum(axis=1) >= 2)
    assert_same_bits(renderer.camlist(s, w, h), lists.words)
    assert 64 * (STACK_N + 1) > (1 + s.desc.n_lights) * 64
    render_full_waves(renderer, s, w, h, 6)


# ------------------------------------------------------------------ ties, single triangles ----
def coincident_scene(first, second, w=32, h=24):
    s = es.eye_scene(w, h)
    a, b = es.at(w, h, -4.0, -4.0, 9.0), es.at(w, h, w + 4.0, -4.0, 9.5)
    c, d = es.at(w, h, w + 4.0, 0.8 * h, 11.0), es.at(w, h, -4.0, 0.8 * h, 10.5)
    for name, albedo in (("upper", first), ("lower", second)):   # the same vertices twice
        s.add_mesh(name, [(a, c, b), (a, d, c)], albedo)   # facing the eye
    s.add_quad_light("lamp", (-2.0, 3.0, -1.0), (-2.0, 3.0, -4.0), (2.0, 3.0, -1.0), (20.0, 20.0, 20.0))
    s.flatten()
    return s


def test_coincident_objects_tie_to_lower_index(renderer):
    """Two objects of one class with the same vertices: every hit is a tie in t, which the
    reference's in-order strict `t < best` scan gives to the first object.  The oracle's frames
    with the albedos swapped differ, so the winner shows."""
    w, h, spp = 32, 24, 6
    red, blue = (0.8, 0.2, 0.1), (0.1, 0.2, 0.8)
    s = coincident_scene(red, blue)
    ref = pyoracle.render(s, w, h, spp)
    swapped = pyoracle.render(coincident_scene(blue, red), w, h, spp)[0]
    assert np.any(ref[0] != swapped)
    render_full_waves(renderer, s, w, h, spp, ref=ref)


def test_single_triangles_beside_three(renderer):
    """classes of 1 (pair j is ray j) and 3 (the magic multiply); the light is a class-1 object too"""
    w, h = 32, 24
    rng = np.random.default_rng(5)
    s = es.eye_scene(w, h)
    s.add_triangle_light("light", (-3.0, 4.0, -6.0), (3.0, 4.0, -6.0), (0.0, 4.0, -12.0), (15.0, 15.0, 15.0))
    for k in range(5):
        c = np.array(es.at(w, h, rng.uniform(2, w - 2), rng.uniform(2, h - 2), rng.uniform(6, 12)))
        s.add_mesh(f"tri_{k}", [c + rng.uniform(-2.5, 2.5, (3, 3))], tuple(rng.uniform(0.2, 0.9, 3)))
    a, b = es.at(w, h, -4.0, 0.6 * h, 8.0), es.at(w, h, w + 4.0, 0.6 * h, 8.0)
    c, d = es.at(w, h, w + 4.0, 0.95 * h, 16.0), es.at(w, h, -4.0, 0.95 * h, 16.0)
    e = es.at(w, h, 0.5 * w, 0.4 * h, 18.0)
    s.add_mesh("floor3", [(a, b, c), (a, c, d), (d, c, e)], (0.6, 0.5, 0.4))
    s.flatten()
    assert sorted(object_counts(s)) == [1] * 6 + [3]
    render_full_waves(renderer, s, w, h, 8)


def test_two_level_original_index_keys(renderer):
    """the small objects of a two-level scene (Cornell around a 24 x 24 sphere mesh): the class
    streams' keys carry the triangles' original indices, merged with the BVH walk's"""
    s, ref = c4_twist_reference()
    render_full_waves(renderer, s, 64, 36, C4_TWIST_SPP, ref=ref, sched=abi.XRT_SCHED_STEP_BVH)
