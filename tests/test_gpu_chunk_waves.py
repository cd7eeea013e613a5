"""The chunk phase with the issue priorities taken in turn (k_step_merged_chunks; chunk_priority in
path_common.h, XRT_CHUNK_PRIO): before each pass a block sets the priority of its waves from its place in
the grid and the passes it has left, so the waves that share a SIMD progress alike.  Priority decides
who issues when and nothing else; a slot's path depends on the slot alone.  So every frame here is held
to the oracle bit for bit, with its segments, shadow rays, draws and rejects, and samples equal.  Every
case forces the phase (XRT_FLAG_CHUNKS); all but the last also force 64 slots per wave, without which a
small render does not start in whole waves.

The shapes are the smallest at which a pass schedule can still go wrong:

* 24 x 18 at 16 spp and 3 visits per pass: deaths spread over many passes and launches, RNG windows
  and refills cross passes.  Under Direct nothing is retired and the 432 slots make two chunks of 256
  and 176, the second with a part-filled and an empty wave (asserted from xrt_test_chunk_plan).  Under
  GI k_camlist retires the pixels no camera ray can hit before the build, so the chunks hold fewer;
  the plan's sizes say how many.  GI also at 1 visit per pass.
* 32 x 24 at 5 spp with material-less blocks (tests/matless_scenes.py cornell_blocks): paths end at
  the blocks early, so waves empty while their siblings stay live and chunks die inside a launch.
* accumulation onto a non-zero frame; row shard 3 of 8.
* two renders in a row on one context, of different live counts.
* 640 x 480 under Direct at 2 spp and 1 visit per pass: more chunks than blocks (asserted first), so
  blocks own two chunks, ownership rotates, and a grid of 1,024 blocks takes all four levels.
* 640 x 480 GI at 8 spp with the layout left to the library: the frame starts a few per cent above
  kMergedLive64 live slots and crosses it inside the phase, so the host's hand-over to the tail
  layouts runs; it must not take more step launches than the grouped schedule (XRT_FLAG_NO_CHUNKS)."""
import functools

import numpy as np
import pytest

import matless_scenes as ms
import pyoracle
from gpu_checks import assert_frame, assert_same_bits, counters_equal, render_pair, renderer  # noqa: F401
from xraytracer_amd import abi, scenes

pytestmark = pytest.mark.gpu

TRACED = ("segments", "shadow_rays", "draws", "rejected")
FORCE = dict(chunks=True, slots_per_wave=64)


def initial_frame(w, h):
    return np.random.default_rng(43).uniform(0.25, 2.0, (h, w, 3)).astype(np.float32)


# name: (scene builder, width, height, spp, render keywords)
CASES = {
    "a_24x18_gi_3_visits": (scenes.cornell, 24, 18, 16, dict(visits_per_launch=3)),
    "a_24x18_direct_two_chunks": (scenes.cornell, 24, 18, 16, dict(visits_per_launch=3, integrator="direct", schedule="step")),
    "a_24x18_gi_1_visit": (scenes.cornell, 24, 18, 16, dict(visits_per_launch=1)),
    "b_32x24_matless_blocks": (ms.cornell_blocks, 32, 24, 5, dict(visits_per_launch=2)),
    "c_accumulate": (scenes.cornell, 64, 48, 4, dict(visits_per_launch=2, initial=initial_frame(64, 48))),
    "d_row_shard_3_of_8": (scenes.cornell, 96, 96, 8, dict(visits_per_launch=2, shard_index=3, shard_count=8)),
    "e_640x480_direct_more_chunks_than_blocks": (scenes.cornell, 640, 480, 2, dict(visits_per_launch=1, interleave=True,
                                                                                   integrator="direct", schedule="step")),
}
ORACLE_KW = ("integrator", "shard_index", "shard_count", "initial")


@functools.lru_cache(maxsize=None)
def reference(name):
    build, w, h, spp, kw = CASES[name]
    s = build(w, h)
    return s, pyoracle.render(s, w, h, spp, **{k: v for k, v in kw.items() if k in ORACLE_KW})


def check(renderer, s, w, h, spp, ref, **kw):
    img, want, st, g = render_pair(renderer, s, w, h, spp, ref=ref, **kw)
    assert g.schedule == abi.XRT_SCHED_STEP_MERGED and g.layout_launches[0] >= 1, list(g.layout_launches)
    assert_frame(img, want)
    counters_equal(g, st, TRACED)
    assert g.samples == st["samples"], (g.samples, st["samples"])
    return img, g


@pytest.mark.parametrize("name", list(CASES))
def test_rotated_priorities_are_the_oracle(renderer, name):
    build, w, h, spp, kw = CASES[name]
    s, ref = reference(name)
    renderer.spp = spp
    renderer._uploaded = None
    plan = renderer.chunk_plan(s, w, h, **FORCE, **{k: v for k, v in kw.items() if k != "initial"})
    sizes = plan["sizes"]
    print(name, "plan", {k: v for k, v in plan.items() if k != "sizes"}, "sizes", sizes[sizes > 0].tolist()[:12])
    assert plan["chunks"] and plan["C"] >= 1
    if name == "a_24x18_direct_two_chunks":   # one partition, class 0: chunks 0 and 8; a part-filled and an empty wave
        assert plan["C"] == 2 and sizes[0] == 256 and sizes[8] == 176, sizes[:16].tolist()
    if name.startswith("e_"):
        assert plan["C"] > plan["blocks"] == 1024, (plan["C"], plan["blocks"])   # some blocks own two chunks
    _, g = check(renderer, s, w, h, spp, ref, **FORCE, **kw)
    print(name, "step launches", g.launches[abi.XRT_K_STEP], "iterations", g.iterations, "layouts", list(g.layout_launches))
    assert sum(g.layout_launches[1:]) == 0   # forced to 64 slots: the phase, then 64-slot rounds only


def test_two_renders_in_a_row_on_one_context(renderer):
    """a larger frame after a smaller one, then the smaller one again, each the oracle's"""
    small, big = "a_24x18_gi_3_visits", "b_32x24_matless_blocks"
    first = None
    for name in (small, big, small):
        build, w, h, spp, kw = CASES[name]
        s, ref = reference(name)
        img, _ = check(renderer, s, w, h, spp, ref, **FORCE, **kw)
        if name == small:
            if first is None:
                first = img
            else:
                assert_same_bits(img, first)


def test_the_phase_crosses_the_threshold_inside_a_launch(renderer):
    """640 x 480 GI at 8 spp, 1 visit per pass, layout left to the library: the live count falls below
    kMergedLive64 inside the phase, the host hands over to the tail layouts, and the chunk phase costs no
    more step launches than the grouped schedule"""
    w, h, spp = 640, 480, 8
    s = scenes.cornell(w, h)
    ref = pyoracle.render(s, w, h, spp)
    kw = dict(visits_per_launch=1, slots_per_wave=0)
    renderer.spp = spp
    renderer._uploaded = None
    plan = renderer.chunk_plan(s, w, h, chunks=True, **kw)
    live = int(plan["sizes"].sum())
    print("plan", {k: v for k, v in plan.items() if k != "sizes"}, "live", live)
    assert plan["chunks"] and 160000 <= live < 1.1 * 160000, live   # kMergedLive64 (wavefront.h)
    img, g = check(renderer, s, w, h, spp, ref, chunks=True, **kw)
    assert g.layout_launches[0] >= 1 and sum(g.layout_launches[1:]) >= 1, list(g.layout_launches)
    one, _, _, f = render_pair(renderer, s, w, h, spp, ref=ref, chunks=False, **kw)
    assert_same_bits(img, one)
    print("step launches", g.launches[abi.XRT_K_STEP], "against", f.launches[abi.XRT_K_STEP], "layouts",
          list(g.layout_launches), list(f.layout_launches))
    assert g.launches[abi.XRT_K_STEP] <= f.launches[abi.XRT_K_STEP]
