"""The cases of tests/render_var_fused_cases.py, checked without a GPU: the flag is bound, the
per-sample radiances the restatement reads rebuild the oracle's frame bit for bit, and the frames
tests/test_gpu_render_var_fused.py renders reach the situations that test relies on — empty and
covered pixels whose Direct samples are not zero, rejected samples beside accepted ones, two shadow
rays per segment, rings that run out, sixteen partitions."""
import os
import re
import types

import numpy as np
import pytest

import camlist_restatement as cr
import render_var_fused_cases as fc
import render_var_restatement as rv
from xraytracer_amd import abi
from xraytracer_amd.renderer import HipRenderer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the ABI ---------------------------------------------------------------------------------
def test_flag_is_bound():
    src = open(os.path.join(ROOT, "include", "xrt.h")).read()
    assert re.search(r"XRT_FLAG_VAR_FUSED\s*=\s*8192u", src)
    assert abi.XRT_FLAG_VAR_FUSED == 8192 and abi.XRT_ABI_VERSION == 14
    others = [v for k, v in vars(abi).items() if k.startswith("XRT_FLAG_") and k != "XRT_FLAG_VAR_FUSED"]
    assert all(v & abi.XRT_FLAG_VAR_FUSED == 0 for v in others)


def test_params_sets_the_flag():
    me = types.SimpleNamespace(spp=4)
    s = fc.scene("cornell_8")
    assert HipRenderer.params(me, s, 8, 6).flags & abi.XRT_FLAG_VAR_FUSED == 0
    p = HipRenderer.params(me, s, 8, 6, fused_var=True, spec=False)
    assert p.flags == abi.XRT_FLAG_VAR_FUSED | abi.XRT_FLAG_NO_SPEC


# ---- the rebuilt frame is the oracle's, on every case the GPU test renders ------------------------
@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_rebuilt_frame_is_the_oracles(name):
    img, var, rec = fc.reference(name)
    ref, cnt = fc.oracle_frame(name)
    assert np.array_equal(bits(img), bits(ref)), name
    assert rec["rejected"] == cnt["rejected"]
    assert np.isfinite(var).all() and (var >= 0).all() and not np.signbit(var).any()
    assert (var > 0).sum() >= 10, name


def test_the_kstep_cases_exist():
    assert all(n in rv.CASES for n in fc.KSTEP_FROM_RV + ("shard", "whitted_lds_65"))


# ---- what the cases are chosen for ---------------------------------------------------------------
def test_cornell_holds_empty_and_covered_pixels_that_direct_lights():
    s = fc.scene("cornell_64")
    empty = cr.empty_pixels(s, 64, 48)
    covered = cr.classes(cr.camera_lists(s, 64, 48))["covered"].reshape(48, 64)
    assert empty.sum() >= 100 and covered.sum() >= 100 and not (empty & covered).any()
    # GI: the empty pixels' samples are all +0, so their variance is
    _, var, _ = fc.reference("merged_gi_64_pairs")
    assert not bits(var)[empty].any()
    # Direct: a miss adds 0.18 per sample, so the records a fused Direct render leaves for them are not zero
    frame, _, _ = fc.reference("merged_direct_64_pairs")
    assert (frame[empty] > 0.1).all()


def test_rejecting_frames_mix_accepted_and_rejected_samples():
    for name in ("rejects_gi", "rejects_direct"):
        _, var, rec = fc.reference(name)
        assert rec["rejected"] > 1000 and rec["mixed"] >= 50, (name, rec)


def test_two_lights_are_sampled():
    s = fc.scene("two_lights")
    assert s.desc.n_lights == 2
    for integ in ("gi", "direct"):
        two, one = fc.oracle_frame(f"two_lights_{integ}")[1], fc._oracle("cornell_64", 64, 48, 3, (("integrator", integ),))[1]
        assert two["shadow_rays"] > 1.5 * one["shadow_rays"], (integ, two["shadow_rays"], one["shadow_rays"])


def test_twists_case_runs_out_of_ring_words():
    _, cnt = fc.oracle_frame("twists")
    assert cnt["draws"] > 624 * 8 * 6   # more than the seeding twist's 624 words per pixel on average


def test_grouped_frame_has_sixteen_partitions():
    _, w, h, _, _, geo, _ = fc.CASES["groups_256"]
    assert w * h // 2048 == 16 and geo["slots_per_wave"] == 64


def test_four_wave_volumetric_case_is_large_enough():
    _, w, h, spp, sem, _, _ = fc.CASES["kstep_vpt_4_waves"]
    assert w * h == 131072 and sem["integrator"] == "vpt" and spp == 2
