"""The merged schedule's step launches in partition groups (step_groups.h, run_fused): while whole
waves run, a round is one k_step_merged launch per group, each on a stream of its own.  Every frame
here is compared bit for bit, counters included, with the oracle's, and with the same render under
XRT_FLAG_NO_OVERLAP (one launch per round on the context's stream).

A frame is grouped when it has at least 16 live-list partitions of 2,048 slots, so the frames are
256 x 128 (16 partitions: two groups) and 384 x 128 (24: the smallest that three groups take; it runs
in three only in a build with XRT_STEP_GROUPS=3 — the shipped default of 2 renders it in two, and
three groups are otherwise covered by the mapping's CPU test alone), at
64 slots per wave and 4 visits per launch so that a 16 spp frame takes many rounds, pixels finish
in different ones (and at 48 spp rings are twisted in-launch).  240 x 128 has 8 partitions and is not grouped.
640 x 480 with the library's own layouts starts grouped and leaves the groups for the layouts of
fewer slots per wave.  The two-level kernel's launches are never grouped."""
import functools

import numpy as np
import pytest

import pyoracle
from gpu_checks import assert_frame, assert_same_bits, counters_equal, render_pair, renderer  # noqa: F401
from xraytracer_amd import abi, scenes

pytestmark = pytest.mark.gpu

SPP = 16
FULL = dict(slots_per_wave=64, visits_per_launch=4)   # whole waves in every launch, many launches
TRACED = ("segments", "shadow_rays", "draws", "rejected")


@functools.lru_cache(maxsize=None)
def cornell_ref(w, h, spp=SPP, **kw):
    s = scenes.cornell(w, h)
    return s, pyoracle.render(s, w, h, spp, **kw)


def grouped_and_flagged(r, scene, w, h, spp, ref, names=TRACED, **kw):
    """the frame rendered in groups and under XRT_FLAG_NO_OVERLAP: both the oracle's, counters
    included; returns the two xrt_stats"""
    img, want, st, g = render_pair(r, scene, w, h, spp, ref=ref, timing=True, **kw)
    assert_frame(img, want)
    counters_equal(g, st, names)
    one, _, _, f = render_pair(r, scene, w, h, spp, ref=ref, timing=True, overlap=False, **kw)
    assert_same_bits(one, img)
    counters_equal(f, st, names)
    assert f.launches[abi.XRT_K_STEP] == f.iterations, (f.launches[abi.XRT_K_STEP], f.iterations)
    return g, f


@pytest.mark.parametrize("w,parts,spp", [(256, 16, SPP), (384, 24, SPP), (256, 16, 48)])
def test_grouped_cornell_full_waves(renderer, w, parts, spp):
    """16 spp draw at most ~270 of a ring's 624 words per pixel, so no ring is twisted after the
    seeding; the 48 spp frame is there for the in-launch twists (rng_twists > path_slots)"""
    s, ref = cornell_ref(w, 128, spp)
    g, f = grouped_and_flagged(renderer, s, w, 128, spp, ref, **FULL)
    assert g.schedule == abi.XRT_SCHED_STEP_MERGED and g.partitions == f.partitions == parts
    assert g.iterations > 8 and g.rng_twists == f.rng_twists
    assert (g.rng_twists > g.path_slots) == (spp == 48), (g.rng_twists, g.path_slots)
    assert g.launches[abi.XRT_K_STEP] > g.iterations
    assert g.launches[abi.XRT_K_STEP] % g.iterations == 0 and g.launches[abi.XRT_K_STEP] // g.iterations in (2, 3)
    assert g.layout_launches[0] == g.launches[abi.XRT_K_STEP] and f.layout_launches[0] == f.iterations
    assert g.kernel_ms[abi.XRT_K_STEP] > 0.0 and f.kernel_ms[abi.XRT_K_STEP] > 0.0


def test_eligibility_boundary(renderer):
    """8 partitions: one octet cannot be dealt to two groups"""
    s, ref = cornell_ref(240, 128)
    img, want, st, g = render_pair(renderer, s, 240, 128, SPP, ref=ref, **FULL)
    assert_frame(img, want)
    counters_equal(g, st, TRACED)
    assert g.partitions == 8 and g.launches[abi.XRT_K_STEP] == g.iterations > 8


def test_join_before_the_smaller_layouts(renderer):
    """the library's own layouts over 640 x 480 at 4 spp: grouped while 64 slots per wave run (about
    165k slots are live once the empty pixels are retired), then the layouts of 32 and fewer slots per
    wave on the context's stream.  At the default 64 visits per launch 4 spp are over in 4 rounds,
    before a poll can change the layout, so the launches are held to 2 visits: the live count then
    falls through every threshold over some twenty rounds, and a poll is at most 3 rounds old."""
    s, ref = cornell_ref(640, 480, 4)
    g, f = grouped_and_flagged(renderer, s, 640, 480, 4, ref, visits_per_launch=2)
    ll = list(g.layout_launches)
    print("layout launches", ll, "spec", g.spec_launches, "iterations", g.iterations)
    assert ll[0] > 0 and sum(ll[1:]) > 0, ll
    assert g.launches[abi.XRT_K_STEP] > g.iterations
    assert sum(ll) == g.launches[abi.XRT_K_STEP]


def two_lights(w, h):
    s = scenes.SceneBundle()
    s.load_obj(scenes.CORNELL_OBJ)
    s.add_quad_light("QuadLight", (343.0, 548.0, 227.0), (343.0, 548.0, 332.0), (213.0, 548.0, 227.0), (25.0, 25.0, 25.0))
    s.add_triangle_light("TriLight", (100.0, 500.0, 100.0), (150.0, 500.0, 100.0), (100.0, 500.0, 150.0), (10.0, 5.0, 2.0))
    s.flatten()
    s.camera = scenes.pinhole(scenes.CORNELL_C2W, 60.0, w, h)
    return s


def test_direct_two_lights(renderer):
    """the Direct build with two shadow rays per segment, on the per-slot schedule (XRT_FLAG_NO_PIXEL)"""
    s = two_lights(256, 128)
    ref = pyoracle.render(s, 256, 128, SPP, integrator="direct")
    g, _ = grouped_and_flagged(renderer, s, 256, 128, SPP, ref, integrator="direct", schedule="step", **FULL)
    assert g.schedule == abi.XRT_SCHED_STEP_MERGED and g.launches[abi.XRT_K_STEP] > g.iterations >= 4


def test_two_level_scene_is_not_grouped(renderer):
    """the two-level kernel (a sphere mesh in the BVH) at 64 slots per wave over 16 partitions: its
    launcher takes the group too, and must keep one launch of every partition per round"""
    w, h, spp = 256, 128, 2
    s = scenes.cornell_spheremesh(w, h, n_theta=24, n_phi=24)
    img, want, st, g = render_pair(renderer, s, w, h, spp, slots_per_wave=64, visits_per_launch=2)
    assert_frame(img, want)
    counters_equal(g, st, TRACED)
    assert g.schedule == abi.XRT_SCHED_STEP_BVH and g.partitions == 16
    assert g.launches[abi.XRT_K_STEP] == g.iterations > 1 and g.layout_launches[0] == g.iterations


def test_row_shard_accumulates_over_negative_zero(renderer):
    """shard 3 of 8 of a 256 x 1024 image (128 rows: 16 partitions), added to an image that holds -0.0"""
    w, h, spp = 256, 1024, 6
    s = scenes.cornell(w, h)
    rng = np.random.default_rng(23)
    init = rng.uniform(0.0, 2.0, (h, w, 3)).astype(np.float32)
    init[rng.random((h, w, 3)) < 0.2] = -0.0
    kw = dict(shard_index=3, shard_count=8, initial=init)
    ref = pyoracle.render(s, w, h, spp, **kw)
    owned = np.zeros(h, bool)
    owned[3::8] = True
    assert np.signbit(init[owned]).sum() > 1000
    img, want, st, g = render_pair(renderer, s, w, h, spp, ref=ref, **kw, **FULL)
    assert_frame(img[owned], want[owned])
    assert_same_bits(img[~owned], init[~owned])
    counters_equal(g, st, TRACED)
    assert g.path_slots == 128 * w and g.partitions == 16 and g.launches[abi.XRT_K_STEP] > g.iterations
    one, _, _, f = render_pair(renderer, s, w, h, spp, ref=ref, overlap=False, **kw, **FULL)
    assert_same_bits(one, img)
    assert f.launches[abi.XRT_K_STEP] == f.iterations


def test_stream_order(renderer):
    """two accumulating device renders back to back behind long work queued on the caller's stream,
    which writes the image last: the group streams start behind the context's, which waits for the
    caller's, and the second render starts behind the first one's joined groups"""
    import torch

    w, h, spp = 256, 128, 4
    s = scenes.cornell(w, h)
    rng = np.random.default_rng(29)
    init = rng.uniform(0.0, 2.0, (h, w, 3)).astype(np.float32)
    once, _ = pyoracle.render(s, w, h, spp, initial=init)
    twice, _ = pyoracle.render(s, w, h, spp, initial=once)
    renderer.spp = spp
    renderer.upload(s)
    init_t = torch.from_numpy(init).to("cuda:0")
    fb = torch.full((h, w, 3), 77.0, dtype=torch.float32, device="cuda:0")
    junk = torch.randn(2048, 2048, device="cuda:0")
    torch.cuda.synchronize()
    for _ in range(6):   # slow work, then the image the renders add to
        junk = junk @ junk
        junk = junk / junk.norm()
    fb.copy_(init_t)
    stream = torch.cuda.current_stream().cuda_stream
    a = renderer.render_device(s, w, h, fb.data_ptr(), after_stream=stream, accumulate=True, **FULL)
    b = renderer.render_device(s, w, h, fb.data_ptr(), after_stream=stream, accumulate=True, **FULL)
    assert_frame(fb.cpu().numpy(), twice)
    for g in (a, b):
        assert g.launches[abi.XRT_K_STEP] > g.iterations
