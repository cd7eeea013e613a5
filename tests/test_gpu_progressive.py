"""Progressive rendering on the GPU (xrt_progressive_*): a frame rendered in passes of n1, n2, ... samples
is, bit for bit, the frame, the variance plane and the path counters of one render at n1 + n2 + ...
samples.  The references are the oracle's and the restatement's for the existing case tables
(tests/render_var_fused_cases.py, tests/render_var_restatement.py), computed once there and shared with
the modules that render the same cases in one shot.  Without the feature the library has no
xrt_progressive_begin and every test here fails."""
import ctypes as C

import numpy as np
import pytest

import pyoracle
import render_var_fused_cases as fc
import render_var_restatement as rv
from gpu_checks import assert_frame, assert_same_bits, counters_equal, read_ppm, run_example, DATA_DIR, words
from xraytracer_amd import abi, scenes
from xraytracer_amd.renderer import HipRenderer

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hr():
    r = HipRenderer(1, device=0)
    yield r
    r.close()


def run_passes(hr, scene, w, h, passes, variance=True, **kw):
    """one session of `passes`; (frame or (frame, variance) after the last pass, its stats, the
    xrt_progressive_state after every pass)"""
    states = []
    with hr.progressive(scene, w, h, variance=variance, **kw) as s:
        for n in passes:
            s.add(n)
            st = s.state
            states.append((st.active, st.spp_done, st.passes, st.resume_twists, st.path_slots))
        out = s.frame()
        stats = s.stats
    return out, stats, states


def splits(name, spp):
    """the passes a case's spp is rendered in"""
    if name == "twists":
        return [(1, 7, 64, 128)]
    both = [tuple(n for n in (1, 1, spp - 2) if n), (spp - 1, 1)]
    return both[:1] if both[0] == both[1] else both   # 2 spp: (1, 1) once


def case_of(name):
    """(scene, w, h, spp, semantics, launch geometry, schedule, reference, oracle) of a case of either table"""
    if name in fc.CASES:
        scene_name, w, h, spp, sem, geo, sched = fc.CASES[name]
        return fc.scene(scene_name), w, h, spp, sem, geo, sched, fc.reference(name), fc.oracle_frame(name)
    _, w, h, spp, sem = rv.CASES[name]
    return rv.scene(name), w, h, spp, sem, {}, abi.XRT_SCHED_STEP, rv.reference(name), rv.oracle_frame(name)


def check_session(hr, name, passes, **more):
    scene, w, h, spp, sem, geo, sched, reference, oracle = case_of(name)
    assert sum(passes) == spp
    (img, var), st, states = run_passes(hr, scene, w, h, passes, **sem, **{**geo, **more})
    print(f"{name} {passes}: schedule {st.schedule} iterations {st.iterations} resume twists {[q[3] for q in states]}")
    assert_frame(img, oracle[0])
    assert_same_bits(img, reference[0], "frame")
    assert_same_bits(var, reference[1], "variance")
    counters_equal(st, oracle[1])
    assert st.samples == st.path_slots * spp
    assert [q[1] for q in states] == list(np.cumsum(passes)) and [q[2] for q in states] == list(range(1, len(passes) + 1))
    return st, states


def spp_of(name):
    return fc.CASES[name][3] if name in fc.CASES else rv.CASES[name][3]


ALL = sorted(fc.CASES) + list(fc.KSTEP_FROM_RV)


# 1. every schedule and layout with a moments build, in two splits
@pytest.mark.parametrize("name,split", [(n, i) for n in ALL for i in range(len(splits(n, spp_of(n))))])
def test_every_schedule_and_layout(hr, name, split):
    st, states = check_session(hr, name, splits(name, spp_of(name))[split])
    assert st.schedule == case_of(name)[6]
    # 3a. every slot holds a whole block after seeding, and no plan keeps more
    assert states[0][3] == 0


# ... the chunk phase has no moments build: a session without the variance option
@pytest.mark.parametrize("interleave", [None, True])
def test_chunk_phase(hr, interleave):
    scene_name, w, h, spp, sem, _, sched = fc.CASES["groups_256"]
    assert (w, h, spp) == (256, 128, 4)
    kw = dict(slots_per_wave=64, visits_per_launch=2, interleave=interleave, **sem)
    ref, cnt = fc.oracle_frame("groups_256")
    img, st, _ = run_passes(hr, fc.scene(scene_name), w, h, (2, 2), variance=False, chunks=True, **kw)
    assert st.schedule == sched
    assert_frame(img, ref)
    counters_equal(st, cnt)
    plain, f, _ = run_passes(hr, fc.scene(scene_name), w, h, (2, 2), variance=False, chunks=False, **kw)
    assert_frame(plain, ref)
    counters_equal(f, cnt)
    assert 0 < st.launches[abi.XRT_K_STEP] < f.launches[abi.XRT_K_STEP]   # the phase ran: several rounds per launch


# ... and the wavefront schedule
@pytest.mark.parametrize("name", ["gi", "direct", "indirect", "normal", "vpt_smoke", "vpt_nee_smoke", "two_level", "shard"])
@pytest.mark.parametrize("split", [0, 1])
def test_wavefront(hr, name, split):
    _, w, h, spp, sem = rv.CASES[name]
    passes = splits(name, spp)[split]
    (img, var), st, _ = run_passes(hr, rv.scene(name), w, h, passes, schedule="wavefront", **sem)
    assert st.schedule == abi.XRT_SCHED_WAVEFRONT
    assert_frame(img, rv.oracle_frame(name)[0])
    assert_same_bits(var, rv.reference(name)[1], "variance")
    counters_equal(st, rv.oracle_frame(name)[1])


# 2. every boundary is a frame
@pytest.fixture(scope="module")
def prefixes():
    """Cornell 64 x 48 GI: per k = 1 .. 5 the oracle's frame and counters at k spp and, from the samples
    of the 5-spp render, the restatement's frame and plane of the first k"""
    w, h = 64, 48
    s = scenes.cornell(w, h)
    pix, rad = rv.samples(s, w, h, 5, integrator="gi")
    out = {}
    for k in range(1, 6):
        frame, var, _ = rv.moments(rad[:, :k])
        out[k] = (pyoracle.render(s, w, h, k, integrator="gi"), frame.reshape(h, w, 3), var.reshape(h, w))
    return s, out


def test_every_boundary_is_a_frame(hr, prefixes):
    s, ref = prefixes
    with hr.progressive(s, 64, 48, variance=True, integrator="gi") as ps:
        for k in range(1, 6):
            st = ps.add(1)
            assert ps.spp_done == k
            if k == 1:
                img = ps.frame(variance=False)   # one sample has no variance: the frame alone
            else:
                img, var = ps.frame()
                assert_same_bits(var, ref[k][2], f"variance at {k} spp")
            assert_frame(img, ref[k][0][0])
            assert_same_bits(img, ref[k][1], f"frame at {k} spp")
            counters_equal(st, ref[k][0][1])


# 3. both resume branches ran
# A resume twists a slot's ring when the pass before left it fewer than rng_keep words.  At the default
# geometry the plan keeps 520 of a block's 624 words and (1, 7, 64, 128) shows both branches (measured:
# resume twists [0, 0, 0, 22] of 48 slots).  With visits_per_launch=1 it keeps 16: a slot is short only if
# its last launch of the pass began with 16 to 23 words ahead.  No slot was over the 3 resumes of
# (1, 7, 64, 128), the 9 of (1, 7, 24 x 8) or the 49 of (4 x 50) (measured: all 0), so this geometry gets
# the same 200 samples one per pass, 199 resumes, where some slots are (measured).
@pytest.mark.parametrize("kw,passes", [({}, (1, 7, 64, 128)), (dict(visits_per_launch=1), (1,) * 200)])
def test_resume_twists_some_slots_and_not_others(hr, kw, passes):
    st, states = check_session(hr, "twists", passes, **kw)
    twisted = [q[3] for q in states]
    assert twisted[0] == 0
    assert any(0 < t < states[0][4] for t in twisted[1:]), twisted


# 4. session rules
def test_frame_repeats_and_denoise_keeps_the_session(hr, prefixes):
    s, ref = prefixes
    with hr.progressive(s, 64, 48, variance=True, integrator="gi") as ps:
        ps.add(2)
        a, av = ps.frame()
        b, bv = ps.frame()
        assert_same_bits(a, b)
        assert_same_bits(av, bv)
        assert_frame(a, ref[2][0][0])
        clean, _ = hr.denoise_var(None, {}, variance=av, width=64, height=48)   # the context's last framebuffer: this frame
        again, _ = hr.denoise_var(a, {}, variance=av)
        assert_same_bits(clean, again)
        assert ps.state.active == 1
        ps.add(3)
        img, var = ps.frame()
        assert_frame(img, ref[5][0][0])
        assert_same_bits(var, ref[5][2])
        assert np.array_equal(hr.tonemap(64, 48, 1.2), pyoracle.tonemap(ref[5][0][0], 1.2))


def test_what_ends_a_session(hr, prefixes):
    s, ref = prefixes
    lib = abi.lib()
    cam = s.camera

    def ended():
        st = abi.XrtStats()
        assert lib.xrt_progressive_add(hr.ctx, 1, C.byref(st)) == abi.XRT_ERR_INVALID
        img = np.zeros((48, 64, 3), np.float32)
        assert lib.xrt_progressive_frame(hr.ctx, abi.fptr(img), None) == abi.XRT_ERR_INVALID
        q = abi.XrtProgressiveState()
        assert lib.xrt_progressive_query(hr.ctx, C.byref(q)) == 0 and q.active == 0

    def render():
        hr.spp = 3
        assert_frame(hr.render(s, 64, 48, integrator="gi"), ref[3][0][0])   # and no state leaks into a one-shot render

    enders = (render,
              lambda: hr._check(lib.xrt_set_camera(hr.ctx, abi.fptr(cam.c2w), C.c_float(cam.scale), C.c_float(cam.aspect)), "camera"),
              lambda: hr.upload(s),
              lambda: lib.xrt_progressive_end(hr.ctx))
    for end in enders:
        ps = hr.progressive(s, 64, 48, integrator="gi")
        ps.add(1)
        assert ps.state.active == 1
        end()
        ended()
    # a fresh begin then works, and a second begin replaces the open session
    ps = hr.progressive(s, 64, 48, integrator="gi")
    ps.add(4)
    ps = hr.progressive(s, 64, 48, integrator="gi")
    assert ps.state.spp_done == 0
    ps.add(2), ps.add(1)
    assert_frame(ps.frame(), ref[3][0][0])
    ps.close()
    ended()


def test_refusals():
    import whitted_scenes as ws

    lib = abi.lib()
    r = HipRenderer(1)
    try:
        s = scenes.cornell(8, 6)
        r.upload(s)
        img, var = np.zeros((6, 8, 3), np.float32), np.zeros((6, 8), np.float32)

        def begin(options=0, **kw):
            return lib.xrt_progressive_begin(r.ctx, C.byref(r.params(s, 8, 6, **kw)), options)

        assert begin(accumulate=True) == abi.XRT_ERR_UNSUPPORTED
        assert begin(slots_per_wave=5) == abi.XRT_ERR_INVALID   # what xrt_render refuses, the same way
        assert begin(integrator="whitted") == abi.XRT_ERR_UNSUPPORTED
        assert begin() == 0
        assert lib.xrt_progressive_frame(r.ctx, abi.fptr(img), None) == abi.XRT_ERR_INVALID   # before any add
        assert lib.xrt_progressive_add(r.ctx, 0, None) == abi.XRT_ERR_INVALID
        assert lib.xrt_progressive_add(r.ctx, 1, None) == 0
        assert lib.xrt_progressive_add(r.ctx, 0xffffffff, None) == abi.XRT_ERR_INVALID   # spp_done would overflow
        assert lib.xrt_progressive_frame(r.ctx, abi.fptr(img), abi.fptr(var)) == abi.XRT_ERR_INVALID   # no variance option
        assert lib.xrt_progressive_frame(r.ctx, abi.fptr(img), None) == 0
        assert begin(abi.XRT_PROGRESSIVE_VARIANCE) == 0
        assert lib.xrt_progressive_add(r.ctx, 1, None) == 0
        assert lib.xrt_progressive_frame(r.ctx, abi.fptr(img), abi.fptr(var)) == abi.XRT_ERR_INVALID   # one sample
        assert lib.xrt_progressive_add(r.ctx, 1, None) == 0
        assert lib.xrt_progressive_frame(r.ctx, abi.fptr(img), abi.fptr(var)) == 0
    finally:
        r.close()
    m = HipRenderer(1, devices=[0, 0])
    try:
        s = scenes.cornell(8, 6)
        m.upload(s)
        assert lib.xrt_progressive_begin(m.ctx, C.byref(m.params(s, 8, 6)), 0) == abi.XRT_ERR_UNSUPPORTED
    finally:
        m.close()


# 5. shards and device memory
def test_shard_leaves_other_rows_zero(hr):
    _, w, h, spp, sem = rv.CASES["shard"]
    (img, var), st, _ = run_passes(hr, rv.scene("shard"), w, h, (1, 3), **sem)
    assert_frame(img, rv.oracle_frame("shard")[0])
    assert_same_bits(var, rv.reference("shard")[1])
    rows = np.arange(12) % 3 == 1
    assert not words(img)[~rows].any() and not words(var)[~rows].any()
    assert (var[rows] > 0).any() and st.samples == 4 * 16 * 4


def test_frame_device_equals_the_host_frame(hr, prefixes):
    import torch

    s, ref = prefixes
    w, h, pad = 64, 48, 64
    n, nv = 3 * w * h, w * h
    f32 = dict(dtype=torch.float32, device="cuda:0")
    out, outv = torch.empty(pad + n + pad, **f32), torch.empty(pad + nv + pad, **f32)
    out.fill_(-7.0)   # queued on the current stream, not waited for
    outv.fill_(-7.0)
    with hr.progressive(s, w, h, variance=True, integrator="gi") as ps:
        ps.add(2), ps.add(3)
        ps.frame_device(out.data_ptr() + 4 * pad, outv.data_ptr() + 4 * pad, after_stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        img, var = ps.frame()
    got, gotv = out.cpu().numpy(), outv.cpu().numpy()
    assert (got[:pad] == -7.0).all() and (got[pad + n:] == -7.0).all()
    assert (gotv[:pad] == -7.0).all() and (gotv[pad + nv:] == -7.0).all()
    assert_same_bits(got[pad:pad + n].reshape(h, w, 3), img)
    assert_same_bits(gotv[pad:pad + nv].reshape(h, w), var)
    assert_frame(img, ref[5][0][0])


# 6. HipRenderer's session methods through examples/progressive.cpp
def test_progressive_in_cpp(tmp_path):
    w, h, passes = 48, 36, (1, 2, 4)
    prefix = tmp_path / "frame"
    out = run_example("progressive", w, h, prefix, *passes, env={"XRT_DATA_DIR": DATA_DIR})
    for done in np.cumsum(passes):
        assert f"spp_done {done}," in out
    total = int(sum(passes))
    s = scenes.cornell(w, h)
    ref, cnt = pyoracle.render(s, w, h, total, integrator="gi")
    assert np.array_equal(read_ppm(tmp_path / f"frame.{total}.ppm", w, h), pyoracle.tonemap(ref, 1.2).astype(np.int64))
    last = out.strip().splitlines()[-1]
    assert f"segments {cnt['segments']} shadow_rays {cnt['shadow_rays']} draws {cnt['draws']} rejected {cnt['rejected']}" in last
    assert (tmp_path / f"frame.{total}.denoised.ppm").exists()
