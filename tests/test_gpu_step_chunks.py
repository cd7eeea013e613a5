"""The merged schedule's whole-wave phase in block-owned chunks (xraytracer_amd/csrc/step_chunks.h,
k_step_merged_chunks, k_chunks_build, k_chunks_scatter; run_chunks in api_render.cpp).  A slot's path
depends on the slot alone, so every frame here is compared bit for bit with the oracle's and with the
same render under XRT_FLAG_NO_CHUNKS, whose per-pixel counters' sums it must share; it must take
fewer step launches than that render.  The cases force the phase (XRT_FLAG_CHUNKS), all but two at 64
slots per wave, at the smallest shapes at which it can still go wrong:

1. 24 x 18 at 3 visits per launch, many passes, paths and RNG windows crossing passes and launches
   (k_camlist retires 176 of its 432 pixels, so it is one full chunk) and 32 x 24, two chunks in one
   class, one part-filled; a row shard; 640 x 480 under the interleaved map (k_camlist retires
   so many of its pixels that 656 chunks are left, fewer than blocks) and the same frame under Direct,
   which retires none: 1,207 chunks on 1,024 blocks, double ownership and rotation (asserted from
   xrt_test_chunk_plan first); a
   scene whose retired pixels the build must drop; Direct; two lights; 48 spp (rings twisted inside
   passes); accumulation onto a non-zero frame.  With slots_per_wave forced to 64 a case cannot hand
   over to a 32-, 16- or 4-slot layout, and the small ones may finish inside the launches the host
   issues before its first poll retires.  So two cases are there for the hand-over: 640 x 480 at
   16 spp and 1 visit per pass with the layout left to the library (it starts at 64 slots by its
   size; a pixel's 16 paths sum to 56 visits on average, a few to under 45 or over 70, and a launch
   is 4 visits, so the live count passes below kMergedLive64, 4 % under the 167,000 slots the frame
   starts with, many launches before it reaches 0), where k_chunks_scatter must hand over to the 32-, 16- or 4-slot layouts and
   k_step_spec (sum(layout_launches[1:]) >= 1); and 256 x 128 at 24 spp forced to 64 slots (16
   partitions, two groups), where grouped rounds must follow the phase (more step launches than
   iterations).
2. the chunks as built (xrt_test_chunk_plan): their number is ceil(live / 256) summed per class, live
   being the slots whose camera list is not empty; every chunk but a class's last is full.
3. two contexts' renders one after the other behind one stream, and both flags together.
4. the automatic rule: which renders take the phase, that more chunks than blocks keep the grouped
   schedule, and the flagship's own frame (800 x 600, 1,024 spp, no flag) against the same render
   under XRT_FLAG_NO_CHUNKS: bits, counters, fewer launches, and the hand-over to the tail layouts."""
import ctypes as C
import functools

import numpy as np
import pytest

import elide_scenes as es
import pyoracle
from gpu_checks import assert_frame, assert_same_bits, counters_equal, render_pair, renderer  # noqa: F401
from xraytracer_amd import abi, scenes
from xraytracer_amd.renderer import HipRenderer

pytestmark = pytest.mark.gpu

SAME = ("samples", "segments", "shadow_rays", "draws", "rejected", "rng_twists")
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
    rng = np.random.default_rng(41)
    return rng.uniform(0.25, 2.0, (h, w, 3)).astype(np.float32)


# name: (scene builder, width, height, spp, render keywords)
CASES = {
    "a_24x18_one_chunk": (scenes.cornell, 24, 18, 6, dict(visits_per_launch=3)),
    "a_32x24_two_chunks": (scenes.cornell, 32, 24, 6, dict(visits_per_launch=3)),
    "b_row_shard_3_of_8": (scenes.cornell, 96, 96, 8, dict(visits_per_launch=2, shard_index=3, shard_count=8)),
    "c_640x480_interleaved": (scenes.cornell, 640, 480, 4, dict(visits_per_launch=2, interleave=True)),
    "c2_640x480_more_chunks_than_blocks": (scenes.cornell, 640, 480, 3, dict(visits_per_launch=1, interleave=True,
                                                                          integrator="direct", schedule="step")),
    "d_retired_pixels": (es.cornell_shifted, 256, 128, 4, dict(visits_per_launch=2, interleave=False)),
    "e_direct": (scenes.cornell, 64, 48, 8, dict(visits_per_launch=1, integrator="direct", schedule="step")),
    "f_two_lights": (two_lights, 64, 48, 8, dict(visits_per_launch=2)),
    "g_48spp_ring_twists": (scenes.cornell, 64, 32, 48, dict(visits_per_launch=4)),
    "h_accumulate": (scenes.cornell, 64, 48, 4, dict(visits_per_launch=2, initial=accumulate_onto(64, 48))),
    "i_grouped_rounds_follow": (scenes.cornell, 256, 128, 24, dict(visits_per_launch=2)),
    "j_640x480_library_layouts": (scenes.cornell, 640, 480, 16, dict(visits_per_launch=1, slots_per_wave=0)),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    build, w, h, spp, kw = CASES[name]
    s = build(w, h)
    return s, pyoracle.render(s, w, h, spp, **{k: v for k, v in kw.items() if k in ("integrator", "shard_index", "shard_count", "initial")})


def expected_chunks(r, s, w, h, kw):
    """chunks per class from the slots that are not retired: slot -> partition -> class p % 8, the
    retired slots being the pixels whose camera list is empty (GI; Direct retires none)"""
    q = {k: v for k, v in kw.items() if k not in ("initial", "slots_per_wave")}
    shard = {k: q[k] for k in ("shard_index", "shard_count") if k in q}
    pix = r.slot_map(s, w, h, chunks=True, slots_per_wave=64, **q)
    n = len(pix)
    live = np.ones(n, bool)
    if q.get("integrator") != "direct":
        lists = r.camlist(s, w, h, **shard)   # pixel order of the shard
        rows = np.arange(shard.get("shard_index", 0), h, shard.get("shard_count", 1))
        local = np.searchsorted(rows, pix // w) * w + pix % w
        live = (lists[local, 0] | lists[local, 1]) != 0
    n_part = min(256, max(1, n // 2048))
    if n_part >= 8:
        n_part &= ~7
    part_cap = (n + n_part - 1) // n_part
    cls = (np.arange(n) // part_cap) % 8
    per_class = [int(live[cls == x].sum()) for x in range(8)]
    return per_class, [(v + 255) // 256 for v in per_class]


@pytest.mark.parametrize("name", list(CASES))
def test_chunk_phase_is_the_oracle_and_the_grouped_render(renderer, name):
    build, w, h, spp, kw = CASES[name]
    s, ref = reference(name)
    force = dict(kw)
    force.setdefault("slots_per_wave", 64)
    forced64 = force["slots_per_wave"] == 64
    renderer.spp = spp
    renderer._uploaded = None
    plan = renderer.chunk_plan(s, w, h, chunks=True, **{k: v for k, v in force.items() if k != "initial"})
    per_class, want_chunks = expected_chunks(renderer, s, w, h, kw)
    print(name, "plan", {k: v for k, v in plan.items() if k != "sizes"}, "live per class", per_class)
    assert plan["chunks"] and plan["passes"] == 4
    assert plan["C"] == sum(want_chunks), (plan["C"], want_chunks)
    sizes = plan["sizes"]
    for x in range(8):   # every chunk of a class full but its last; none beyond
        got = sizes[x::8]
        full, rest = divmod(per_class[x], 256)
        want = [256] * full + ([rest] if rest else [])
        assert got[:len(want)].tolist() == want and not got[len(want):].any(), (x, want, got[:len(want) + 2])
    if name.startswith("a_32"):
        assert plan["C"] == 2 and plan["blocks"] == 16 and sizes[0] == 256 and 0 < sizes[8] < 256
    if name.startswith("c2_"):
        assert plan["C"] > plan["blocks"] == 1024, (plan["C"], plan["blocks"])   # some blocks own two chunks
    if name.startswith("d_"):
        assert sum(per_class) < 0.8 * w * h   # the build dropped the retired pixels

    img, want, st, g = render_pair(renderer, s, w, h, spp, ref=ref, chunks=True, **force)
    assert g.schedule == abi.XRT_SCHED_STEP_MERGED and g.slots_per_wave == 64   # the first launch's layout
    assert_frame(img, want)
    counters_equal(g, st, TRACED)
    one, _, _, f = render_pair(renderer, s, w, h, spp, ref=ref, chunks=False, **force)
    assert_same_bits(img, one)
    for k in SAME:
        assert getattr(g, k) == getattr(f, k), (k, getattr(g, k), getattr(f, k))
    print(name, "step launches", g.launches[abi.XRT_K_STEP], "against", f.launches[abi.XRT_K_STEP],
          "iterations", g.iterations, f.iterations, "layouts", list(g.layout_launches))
    assert 0 < g.launches[abi.XRT_K_STEP] < f.launches[abi.XRT_K_STEP]
    if forced64:   # the scatter can only hand over to 64-slot rounds
        assert sum(g.layout_launches[1:]) == 0
    else:          # ... to the tail layouts, below kMergedLive64
        assert g.layout_launches[0] >= 1 and sum(g.layout_launches[1:]) >= 1, list(g.layout_launches)
    if name.startswith("i_"):   # grouped rounds (two launches each) after the scatter
        assert g.launches[abi.XRT_K_STEP] > g.iterations, (g.launches[abi.XRT_K_STEP], g.iterations)
    if name.startswith("g_"):
        assert g.rng_twists - g.path_slots > 0


def test_two_contexts_behind_one_stream():
    """two contexts render the chunk phase one after the other behind the work of one stream: the
    frames they render alone"""
    import torch

    w, h, spp = 64, 48, 6
    a, b = scenes.cornell(w, h), two_lights(w, h)
    kw = dict(chunks=True, slots_per_wave=64, visits_per_launch=2)
    ra, rb = HipRenderer(spp, device=0), HipRenderer(spp, device=0)
    try:
        alone_a, alone_b = ra.render(a, w, h, **kw), rb.render(b, w, h, **kw)
        fa = torch.full((h, w, 3), 7.0, dtype=torch.float32, device="cuda:0")
        fb = torch.full((h, w, 3), 9.0, dtype=torch.float32, device="cuda:0")
        junk = torch.randn(1024, 1024, device="cuda:0")
        for _ in range(4):
            junk = junk @ junk
            junk = junk / junk.norm()
        stream = torch.cuda.current_stream().cuda_stream
        ra.render_device(a, w, h, fa.data_ptr(), after_stream=stream, **kw)
        rb.render_device(b, w, h, fb.data_ptr(), after_stream=stream, **kw)
        ra.render_device(a, w, h, fa.data_ptr(), after_stream=stream, **kw)
        assert_same_bits(fa.cpu().numpy(), alone_a)
        assert_same_bits(fb.cpu().numpy(), alone_b)
        assert_frame(alone_a, pyoracle.render(a, w, h, spp)[0])
    finally:
        ra.close()
        rb.close()


def test_no_chunks_wins(renderer):
    """both flags: the grouped schedule (256 x 128: 16 partitions, two groups)"""
    w, h, spp = 256, 128, 4
    s = scenes.cornell(w, h)
    renderer.spp = spp
    renderer._uploaded = None
    renderer.upload(s)
    p = renderer.params(s, w, h, slots_per_wave=64, visits_per_launch=2)
    p.flags |= abi.XRT_FLAG_CHUNKS | abi.XRT_FLAG_NO_CHUNKS
    plan = np.zeros(5, np.uint32)
    assert abi.lib().xrt_test_chunk_plan(renderer.ctx, C.byref(p), abi.u32ptr(plan), None, 0) == abi.XRT_OK
    assert not plan.any()
    img = np.zeros((h, w, 3), np.float32)
    g = abi.XrtStats()
    assert abi.lib().xrt_render(renderer.ctx, C.byref(p), abi.fptr(img), C.byref(g)) == abi.XRT_OK
    assert g.launches[abi.XRT_K_STEP] > g.iterations
    assert_frame(img, pyoracle.render(s, w, h, spp)[0])
    # and without the flags no render of this size takes the phase
    assert not renderer.chunk_plan(s, w, h)["chunks"]
    assert not renderer.chunk_plan(s, w, h, slots_per_wave=64, visits_per_launch=2)["chunks"]


def test_the_flagship_takes_chunks_by_the_rule(renderer):
    """800 x 600 at 1,024 spp with no flag: 4 passes and no more chunks than blocks (k_camlist leaves
    1,024 chunks for 1,024 blocks); not at 64 spp, nor below the spp that gives 4 passes.  Then the frame
    itself against the same render on the grouped schedule."""
    s = scenes.cornell(800, 600)
    renderer._uploaded = None
    renderer.spp = 1024
    plan = renderer.chunk_plan(s, 800, 600)
    print("flagship plan", {k: v for k, v in plan.items() if k != "sizes"})
    assert plan["chunks"] and plan["passes"] == 4 and plan["blocks"] == 1024 and 1000 <= plan["C"] <= 1024
    img = renderer.render(s, 800, 600)
    g = renderer.stats
    one = renderer.render(s, 800, 600, chunks=False)
    f = renderer.stats
    assert_same_bits(img, one)
    assert np.all(np.isfinite(img))
    for k in SAME:
        assert getattr(g, k) == getattr(f, k), (k, getattr(g, k), getattr(f, k))
    print("flagship step launches", g.launches[abi.XRT_K_STEP], "against", f.launches[abi.XRT_K_STEP], "iterations",
          g.iterations, f.iterations, "layouts", list(g.layout_launches), list(f.layout_launches))
    assert 3 <= g.launches[abi.XRT_K_STEP] < f.launches[abi.XRT_K_STEP]
    assert g.layout_launches[0] >= 1 and sum(g.layout_launches[1:]) >= 1
    assert f.launches[abi.XRT_K_STEP] > f.iterations   # XRT_FLAG_NO_CHUNKS: grouped rounds
    renderer.spp = 256   # two passes by the quarter rule: fewer than XRT_CHUNK_PASSES
    assert not renderer.chunk_plan(s, 800, 600)["chunks"]
    renderer.spp = 1024
    assert not renderer.chunk_plan(s, 800, 600, chunks=False)["chunks"]
    assert not renderer.chunk_plan(s, 800, 600, interleave=False)["chunks"]
    renderer.spp = 64
    assert not renderer.chunk_plan(s, 800, 600)["chunks"]


def test_more_chunks_than_blocks_keep_the_grouped_schedule_by_the_rule(renderer):
    """640 x 480 under Direct retires no pixel: 1,207 chunks.  By the rule (1,024 spp, no flag) the plan
    has the phase, the build finds more chunks than blocks and the render keeps the grouped schedule;
    forced, it runs (case c2 above)."""
    s = scenes.cornell(640, 480)
    renderer._uploaded = None
    renderer.spp = 1024
    kw = dict(integrator="direct", schedule="step")
    plan = renderer.chunk_plan(s, 640, 480, **kw)
    assert not plan["chunks"] and plan["passes"] == 4 and plan["C"] > 1024 and plan["blocks"] == 0
    forced = renderer.chunk_plan(s, 640, 480, chunks=True, **kw)
    assert forced["chunks"] and forced["blocks"] == 1024 and forced["C"] == plan["C"]
