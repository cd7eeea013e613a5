"""First-hit guide buffers on the GPU (xrt_render_aov, aov.hip) against the restatement
(tests/aov_restatement.py): all five planes bit for bit, the stats fields for equality.  The
cases and the situations they are chosen for are in tests/aov_restatement.py and checked without
a GPU in tests/test_aov_restatement.py."""
import ctypes as C

import numpy as np
import pytest

import aov_restatement as ar
import multi_stats
import pyoracle
import whitted_bvh_scenes as wb
from gpu_checks import assert_same_bits, read_ppm, render_rc, run_example, words
from xraytracer_amd import abi
from xraytracer_amd.renderer import HipRenderer

pytestmark = pytest.mark.gpu


def assert_planes(got, ref, names=ar.PLANES):
    for k in names:
        assert_same_bits(got[k], ref[k], k)


def check_case(name, devices=None, want_kernel=None):
    """CASES[name] on the GPU: planes and counters against the restatement"""
    _, w, h, spp, kw = ar.CASES[name]
    ref, cnt, per = ar.reference(name)
    r = HipRenderer(spp, devices=devices)
    try:
        got = r.render_aov(ar.scene(name), w, h, **kw)
        st = r.stats
        assert {k: int(getattr(st, k)) for k in ar.COUNTERS} == {k: int(cnt[k]) for k in ar.COUNTERS}
        assert st.launches[abi.XRT_K_STEP] == (2 if devices else 1) and st.launches[abi.XRT_K_FINISH] == 0
        assert_planes(got, ref)
    finally:
        r.close()
    return got, cnt, per


# 1. each scene kind over the LDS-resident scene: triangles, spheres (scanned, sphere BVH), mixed
#    with a medium box, an emitter, metal and glass first hits
@pytest.mark.parametrize("name", ar.LDS_KINDS)
def test_scene_kinds(name):
    check_case(name)


# 2. triangle scenes beyond LDS: through the BVH, with no flag (two-level, one-level, ties)
@pytest.mark.parametrize("name", ar.BVH_KINDS)
def test_bvh_scenes(name):
    check_case("bvh_" + name)
    # the same scene is refused by a Whitted render without XRT_FLAG_WHITTED_BVH: the guide pass
    # took the BVH kernel by itself
    rc, _ = render_rc(ar.scene("bvh_" + name), 24, 18, 1, integrator="whitted")
    assert rc == abi.XRT_ERR_UNSUPPORTED


# 3. the ordered sum across windows, runs of the sum buffer and ring chunks
@pytest.mark.parametrize("spp", ar.EDGE_SPP)
def test_window_edges(spp):
    check_case(f"edge_{spp}")


# 4. sharding: rows 1, 4, 7, ... of example(48, 36); the other rows 0 / -1
def test_row_shard():
    got, _, per = check_case("example_shard")
    other = np.ones(36, bool)
    other[sorted({i for i, _ in per["pix"]})] = False
    for k in ("albedo", "normal", "depth", "alpha"):
        assert not words(got[k][other]).any()
    assert (got["object"][other] == -1).all()


# 5. multi-device context over one GPU listed twice
def test_multi_device_context():
    check_case("example", devices=[0, 0])
    check_case("example_shard", devices=[0, 0])
    check_case("bvh_glass", devices=[0, 0])


def test_multi_device_stats_are_the_devices_sums():
    """xrt_stats of a two-device guide pass against its two row shards on one device: every
    counter of the structure the sum, the schedule's description device 0's (multi_stats)"""
    from xraytracer_amd import scenes

    s = scenes.cornell(32, 24)
    one, two = HipRenderer(2), HipRenderer(2, devices=[0, 0])
    try:
        parts = []
        for i in range(2):
            one.render_aov(s, 32, 24, shard_index=i, shard_count=2)
            parts.append(multi_stats.counters(one.stats))
        assert parts[0]["samples"] == parts[1]["samples"] == 32 * 12 * 2
        assert parts[0]["schedule"] == abi.XRT_SCHED_AOV
        two.render_aov(s, 32, 24)
        assert multi_stats.counters(two.stats) == multi_stats.combined(parts)
    finally:
        one.close()
        two.close()


# 6. plane subsets: supplied planes equal the full call's, nothing else is written
@pytest.mark.parametrize("subset", [("depth", "object"), ("albedo",)])
def test_plane_subsets(subset):
    _, w, h, spp, _ = ar.CASES["example"]
    ref, cnt, _ = ar.reference("example")
    r = HipRenderer(spp)
    try:
        got = r.render_aov(ar.scene("example"), w, h, planes=subset)
        assert tuple(got) == subset
        assert_planes(got, ref, subset)
        assert int(r.stats.samples) == cnt["samples"]
        # the same through the C call, with a guard pattern in separate buffers the call is not given
        guard = {k: np.full(ref[k].shape, 0x5A5A5A5A, np.uint32) for k in ar.PLANES}
        mine = {k: np.zeros(ref[k].shape, ref[k].dtype) for k in subset}
        bufs = abi.XrtAovBuffers(**{k: a.ctypes.data for k, a in mine.items()})
        p = r.params(ar.scene("example"), w, h)
        assert abi.lib().xrt_render_aov(r.ctx, C.byref(p), C.byref(bufs), None) == 0
        assert_planes(mine, ref, subset)
        assert all((g == 0x5A5A5A5A).all() for g in guard.values())
    finally:
        r.close()


def test_plane_subset_on_the_device_leaves_other_memory_alone():
    """depth + object into one torch allocation that also holds guard words round them"""
    import torch

    _, w, h, spp, _ = ar.CASES["example"]
    ref, _, _ = ar.reference("example")
    n = w * h
    pad = 64
    buf = torch.full((pad + n + pad + n + pad,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    base = buf.data_ptr()
    r = HipRenderer(spp)
    try:
        r.render_aov_device(ar.scene("example"), w, h, dict(depth=base + 4 * pad, object=base + 4 * (2 * pad + n)),
                            after_stream=torch.cuda.current_stream().cuda_stream)
    finally:
        r.close()
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    for a, b in ((0, pad), (pad + n, 2 * pad + n), (2 * pad + 2 * n, 3 * pad + 2 * n)):
        assert (host[a:b] == 0x5A5A5A5A).all()
    assert np.array_equal(host[pad:pad + n].view(np.uint32), words(ref["depth"]).reshape(-1))
    assert np.array_equal(host[2 * pad + n:2 * pad + 2 * n], ref["object"].reshape(-1))


# 7. the device entry point into torch tensors on the current stream
@pytest.mark.parametrize("devices", [None, [0, 0]])
def test_device_entry_point(devices):
    import torch

    _, w, h, spp, _ = ar.CASES["example"]
    ref, cnt, _ = ar.reference("example")
    t = {k: torch.full(ref[k].shape, 7, dtype=torch.int32 if k == "object" else torch.float32, device="cuda:0")
         for k in ar.PLANES}   # written on the current stream right before the call: the pass must wait for it
    r = HipRenderer(spp, devices=devices)
    try:
        host = r.render_aov(ar.scene("example"), w, h)
        st = r.render_aov_device(ar.scene("example"), w, h, {k: v.data_ptr() for k, v in t.items()},
                                 after_stream=torch.cuda.current_stream().cuda_stream)
        assert {k: int(getattr(st, k)) for k in ar.COUNTERS} == {k: int(cnt[k]) for k in ar.COUNTERS}
    finally:
        r.close()
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in t.items()}
    assert_planes(got, host)
    assert_planes(got, ref)


# 8. the guide pass saw the Normal integrator's rays: NormalIntegrator returns 0.5f * (ns + 1.0f) on
#    a hit and 0 on a miss, so its frame is 0.5 * (normal + alpha) up to the rounding of the two
#    sums: with values in [-1, 1], spp = 3 additions, one halving, one add and one division on each
#    side, at most 8 roundings of at most 2^-24 each
def test_normal_integrator_tie_in():
    _, w, h, spp, _ = ar.CASES["example"]
    r = HipRenderer(spp)
    try:
        s = ar.scene("example")
        g = r.render_aov(s, w, h)
        frame = r.render(s, w, h, integrator="normal")
        assert r.stats.schedule == abi.XRT_SCHED_PIXEL and r.stats.rejected == 0
    finally:
        r.close()
    miss, full = g["alpha"] == 0, g["alpha"] == 1
    assert miss.any() and full.any() and (~miss & ~full).any()
    assert not words(frame[miss]).any()           # the miss colour exactly: no sample of the pixel hit
    assert (frame[full] >= 0).all() and (frame[full].sum(axis=-1) > 0).all()
    want = 0.5 * (g["normal"].astype(np.float64) + g["alpha"].astype(np.float64)[..., None])
    assert np.abs(frame - want).max() <= 8 * 2.0 ** -24
    assert ((frame != 0).any(axis=-1) == (g["alpha"] > 0)).all()   # partially covered pixels too


# 9. refusals
def aov_rc(scene, w, h, spp, planes=ar.PLANES, upload=True, **kw):
    r = HipRenderer(spp)
    try:
        if upload:
            r.upload(scene)
        p = r.params(scene, w, h, **kw)
        out = {k: np.zeros((h, w, 3) if k in ("albedo", "normal") else (h, w), np.int32 if k == "object" else np.float32)
               for k in planes}
        bufs = abi.XrtAovBuffers(**{k: a.ctypes.data for k, a in out.items()})
        rc = abi.lib().xrt_render_aov(r.ctx, C.byref(p), C.byref(bufs), None)
        return rc, abi.lib().xrt_last_error(r.ctx).decode()
    finally:
        r.close()


def test_large_mixed_scene_is_unsupported():
    rc, msg = aov_rc(wb.mixed_beyond_lds(24, 18), 24, 18, 1)
    assert rc == abi.XRT_ERR_UNSUPPORTED and "mixed" in msg


def test_accumulate_is_unsupported():
    rc, msg = aov_rc(ar.scene("example"), 48, 36, 1, accumulate=True)
    assert rc == abi.XRT_ERR_UNSUPPORTED and "ACCUMULATE" in msg


def test_no_plane_is_invalid():
    rc, _ = aov_rc(ar.scene("example"), 48, 36, 1, planes=())
    assert rc == abi.XRT_ERR_INVALID


def test_render_before_upload_is_a_state_error():
    rc, _ = aov_rc(ar.scene("example"), 48, 36, 1, upload=False)
    assert rc == abi.XRT_ERR_STATE


# 10. metal and glass scenes are accepted whatever integrator the parameters name
def test_integrator_and_depth_are_ignored():
    _, w, h, spp, _ = ar.CASES["glass_3"]
    ref, _, _ = ar.reference("glass_3")
    r = HipRenderer(spp)
    try:
        got = r.render_aov(ar.scene("glass_3"), w, h, integrator="gi", max_depth=77, schedule="wavefront")
        assert_planes(got, ref)
    finally:
        r.close()


# 11. timing: the launch is timed as XRT_K_STEP
def test_timing_flag():
    _, w, h, spp, _ = ar.CASES["example"]
    r = HipRenderer(spp)
    try:
        r.render_aov(ar.scene("example"), w, h, timing=True)
        assert r.stats.kernel_ms[abi.XRT_K_STEP] > 0 and r.stats.kernel_ms[abi.XRT_K_SEED] > 0
        r.render_aov(ar.scene("example"), w, h)
        assert r.stats.kernel_ms[abi.XRT_K_STEP] == 0
    finally:
        r.close()


# 12. examples/aov.cpp through the C++ API (HipRenderer::renderGuides)
def test_aov_example_ppm(tmp_path):
    _, w, h, spp, _ = ar.CASES["example"]
    ref, _, _ = ar.reference("example")
    prefix = tmp_path / "guides"
    run_example("aov", w, h, spp, prefix)
    half = np.float32(0.5) * (ref["normal"] + np.float32(1.0))   # 0.5f * (ns + 1.0f)
    assert np.array_equal(read_ppm(tmp_path / "guides.normal.ppm", w, h), pyoracle.tonemap(half, 1.2).astype(np.int64))
    assert np.array_equal(read_ppm(tmp_path / "guides.albedo.ppm", w, h),
                          pyoracle.tonemap(ref["albedo"], 1.2).astype(np.int64))
