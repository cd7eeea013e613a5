"""Pixels interleaved across the merged schedule's path slots (xraytracer_amd/csrc/slot_map.h,
plan_render): slot s renders pixel s * A mod n of the shard, so a wave's 64 slots sample the whole
image.  A slot's path depends on its own pixel and RNG stream only, so every frame here is compared
bit for bit with the oracle's and with the same render under XRT_FLAG_NO_INTERLEAVE, and the
per-pixel counters' sums must be the row-major render's.

1. the permutation forced (XRT_FLAG_INTERLEAVE) at 64 slots per wave and 4 visits per launch: sizes
   that are and are not multiples of 64, a prime slot count, a power of two, Direct, a row shard,
   accumulation onto a non-zero frame, two lights;
2. forced in the layouts of 16 and 4 slots per wave, with speculative starts (k_step_spec) and
   without: the camera lists, the covering shortcut and the retired pixels under the map;
3. the map itself (xrt_test_slot_map): which renders get it, and that it is the restated one;
4. forced together with the partition groups of tests/test_gpu_step_groups.py."""
import ctypes as C
import functools

import numpy as np
import pytest

import pyoracle
from gpu_checks import assert_frame, assert_same_bits, counters_equal, render_pair, renderer  # noqa: F401
from slot_map_restatement import pixels
from xraytracer_amd import abi, scenes

pytestmark = pytest.mark.gpu

FULL = dict(slots_per_wave=64, visits_per_launch=4)
SAME = ("samples", "segments", "shadow_rays", "draws", "rejected", "rng_twists", "iterations")
TRACED = ("segments", "shadow_rays", "draws", "rejected")


def two_lights(w, h):
    """the two-light Cornell box of tests/test_gpu_trace_classes.py"""
    s = scenes.SceneBundle()
    s.load_obj(scenes.CORNELL_OBJ)
    s.add_quad_light("QuadLight", (343.0, 548.0, 227.0), (343.0, 548.0, 332.0), (213.0, 548.0, 227.0), (25.0, 25.0, 25.0))
    s.add_quad_light("SideLight", (1.0, 200.0, 200.0), (1.0, 300.0, 200.0), (1.0, 200.0, 300.0), (9.0, 12.0, 15.0))
    s.flatten()
    s.camera = scenes.pinhole(scenes.CORNELL_C2W, 60.0, w, h)
    return s


def accumulate_onto(w, h):
    rng = np.random.default_rng(10)
    return rng.uniform(0.25, 2.0, (h, w, 3)).astype(np.float32)


# name: (scene builder, width, height, spp, render keywords)
CASES = {
    "a_64x48": (scenes.cornell, 64, 48, 8, {}),
    "b_37x29_odd": (scenes.cornell, 37, 29, 8, {}),
    "c_1201x1_prime": (scenes.cornell, 1201, 1, 4, {}),
    "d_64x64_power_of_two": (scenes.cornell, 64, 64, 4, {}),
    "e_direct": (scenes.cornell, 64, 48, 8, dict(integrator="direct", schedule="step")),
    "f_row_shard_3_of_8": (scenes.cornell, 64, 96, 4, dict(shard_index=3, shard_count=8)),
    "g_accumulate": (scenes.cornell, 64, 48, 4, dict(initial=accumulate_onto(64, 48))),
    "h_two_lights": (two_lights, 64, 48, 8, {}),
}


def forced_and_identity(r, scene, w, h, spp, kw, names=TRACED):
    """the frame with the permutation forced: the oracle's, and the bits and counters of the same
    render under the row-major map; returns the two xrt_stats"""
    img, want, st, g = render_pair(r, scene, w, h, spp, interleave=True, **kw)
    assert g.schedule == abi.XRT_SCHED_STEP_MERGED
    assert_frame(img, want)
    counters_equal(g, st, names)
    one, _, _, f = render_pair(r, scene, w, h, spp, ref=(want, st), interleave=False, **kw)
    assert_same_bits(img, one)
    for k in SAME:
        assert getattr(g, k) == getattr(f, k), (k, getattr(g, k), getattr(f, k))
    return g, f


@pytest.mark.parametrize("name", list(CASES))
def test_forced_interleave_is_the_oracle_and_the_identity_render(renderer, name):
    build, w, h, spp, kw = CASES[name]
    s = build(w, h)
    g, _ = forced_and_identity(renderer, s, w, h, spp, dict(kw, **FULL))
    assert (g.slots_per_wave, g.visits_per_launch) == (64, 4) and g.iterations > 1
    shard = {k: kw[k] for k in ("shard_index", "shard_count") if k in kw}
    m = renderer.slot_map(s, w, h, interleave=True, **{k: v for k, v in kw.items() if k != "initial"}, **FULL)
    assert np.array_equal(m, pixels(w, h, **shard)) and not np.array_equal(m, pixels(w, h, interleave=False, **shard))


@pytest.mark.parametrize("spw,spec", [(16, True), (16, False), (4, True)])
def test_group_layouts_and_camera_lists(renderer, spw, spec):
    s = scenes.cornell(40, 30)
    g, f = forced_and_identity(renderer, s, 40, 30, 9, dict(slots_per_wave=spw, spec=spec, timing=True))
    if spec:
        assert g.spec_launches == g.launches[abi.XRT_K_STEP] > 0
    else:
        assert g.spec_launches == 0 and g.launches[abi.XRT_K_STEP] > 0
    assert f.spec_launches == g.spec_launches


def test_which_renders_get_the_map(renderer):
    s = scenes.cornell(64, 48)
    rowmajor = np.arange(64 * 48, dtype=np.uint32)
    assert np.array_equal(renderer.slot_map(s, 64, 48), rowmajor)   # below the whole-wave layout's size
    assert np.array_equal(renderer.slot_map(s, 64, 48, interleave=False), rowmajor)
    assert np.array_equal(renderer.slot_map(s, 64, 48, interleave=False, **FULL), rowmajor)
    forced = renderer.slot_map(s, 64, 48, interleave=True)
    assert not np.array_equal(forced, rowmajor) and np.array_equal(np.sort(forced), rowmajor)
    assert np.array_equal(forced, pixels(64, 48))
    # the wavefront schedule and the pixel schedule know the row-major map only, whatever the flag says
    assert np.array_equal(renderer.slot_map(s, 64, 48, interleave=True, schedule="wavefront"), rowmajor)
    assert np.array_equal(renderer.slot_map(s, 64, 48, interleave=True, integrator="direct"), rowmajor)
    # both flags: the row-major map wins
    p = renderer.params(s, 64, 48)
    p.flags |= abi.XRT_FLAG_INTERLEAVE | abi.XRT_FLAG_NO_INTERLEAVE
    out = np.zeros(64 * 48, np.uint32)
    assert abi.lib().xrt_test_slot_map(renderer.ctx, C.byref(p), abi.u32ptr(out)) == abi.XRT_OK
    assert np.array_equal(out, rowmajor)


def test_the_flagship_frame_is_interleaved_by_the_rule(renderer):
    """800 x 600 with no flag (no render needed): the restated permutation, word for word, and the
    same for its row shards of 8 (60,000 slots, the smallest shard the rule interleaves); a shard of
    16 keeps the row-major map"""
    s = scenes.cornell(800, 600)
    m = renderer.slot_map(s, 800, 600)
    rowmajor = np.arange(800 * 600, dtype=np.uint32)
    assert np.array_equal(np.sort(m), rowmajor)
    assert np.array_equal(m, pixels(800, 600))
    assert np.array_equal(renderer.slot_map(s, 800, 600, interleave=False), rowmajor)
    sh = renderer.slot_map(s, 800, 600, shard_index=3, shard_count=8)
    assert np.array_equal(sh, pixels(800, 600, 3, 8)) and not np.array_equal(sh, pixels(800, 600, 3, 8, interleave=False))
    sh = renderer.slot_map(s, 800, 600, shard_index=0, shard_count=16)
    assert np.array_equal(sh, pixels(800, 600, 0, 16, interleave=False))


def test_two_level_scene_forced(renderer):
    """the two-level kernel (a sphere mesh in the BVH) over interleaved slots: by the rule only frames
    that start in its whole-wave layout are, so the small frame is forced"""
    w, h, spp = 96, 64, 2
    s = scenes.cornell_spheremesh(w, h, n_theta=24, n_phi=24)
    kw = dict(slots_per_wave=64, visits_per_launch=2)
    img, want, st, g = render_pair(renderer, s, w, h, spp, interleave=True, **kw)
    assert g.schedule == abi.XRT_SCHED_STEP_BVH
    assert_frame(img, want)
    counters_equal(g, st, TRACED)
    assert np.array_equal(renderer.slot_map(s, w, h, interleave=True, **kw), pixels(w, h))
    assert np.array_equal(renderer.slot_map(s, w, h, **kw), pixels(w, h, interleave=False))
    big = renderer.slot_map(s, 1920, 1080)   # C4's frame: interleaved by the rule
    assert np.array_equal(big, pixels(1920, 1080))


@functools.lru_cache(maxsize=None)
def cornell_ref(w, h, spp):
    s = scenes.cornell(w, h)
    return s, pyoracle.render(s, w, h, spp)


def test_groups_and_interleave_together(renderer):
    """tests/test_gpu_step_groups.py's setup, 640 x 480 at 4 spp and 2 visits per launch: grouped
    launches on streams of their own while whole waves run, over interleaved slots"""
    s, ref = cornell_ref(640, 480, 4)
    img, want, st, g = render_pair(renderer, s, 640, 480, 4, ref=ref, interleave=True, visits_per_launch=2)
    assert_frame(img, want)
    counters_equal(g, st, TRACED)
    assert g.launches[abi.XRT_K_STEP] > g.iterations
