"""xrt_render_var's cases, checked without a GPU on the restatement alone (tests/render_var_restatement.py):
the per-sample radiances it reads rebuild the oracle's frame bit for bit, the frames
tests/test_gpu_render_var.py compares with the device's reach the situations that test relies on,
and the sample variance serves the variance-guided filter better than its spatial estimate does."""
import ctypes as C

import numpy as np
import pytest

import aov_restatement as ar
import denoise_var_restatement as dv
import pyoracle
import render_var_restatement as rv
from xraytracer_amd import abi, scenes


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- the ABI ---------------------------------------------------------------------------------
def test_both_entry_points_are_bound():
    assert abi.XRT_ABI_VERSION == 14
    for name in ("xrt_render_var", "xrt_render_var_device"):
        assert name in abi.SIGNATURES and hasattr(abi.lib(), name)
    assert len(abi.SIGNATURES["xrt_render_var"][1]) == 5 and len(abi.SIGNATURES["xrt_render_var_device"][1]) == 6


def test_null_context_is_rejected_without_a_gpu():
    lib = abi.lib()
    p = abi.XrtRenderParams(abi.XRT_INTEGRATOR_GI, 4, 4, 4, 2, 0, 1, 0, 0, 0)
    img, var = np.zeros((4, 4, 3), np.float32), np.zeros((4, 4), np.float32)
    assert lib.xrt_render_var(None, C.byref(p), abi.fptr(img), abi.fptr(var), None) == -1
    assert lib.xrt_render_var_device(None, C.byref(p), None, None, None, None) == -1
    assert lib.xrt_render_var(None, None, None, None, None) == -1


# ---- the arithmetic on values worked out by hand ------------------------------------------------
def test_moments_on_hand_values():
    one = np.float32(1.0)
    rad = np.array([[[1, 1, 1], [1, 1, 1], [1, 1, 1]],                   # constant: l = lum(1, 1, 1), v may round
                    [[0, 0, 0], [0, 0, 0], [0, 0, 0]],                   # black: exactly +0
                    [[1, 1, 1], [np.nan, 0, 0], [3, 3, 3]],              # one reject: n stays 3
                    [[-1, 0, 0], [0, np.inf, 0], [np.nan, 0, 0]]], np.float32)   # all rejected: +0
    frame, var, rec = rv.moments(rad)
    l1 = rv.lum(np.array([1, 1, 1], np.float32))
    l3 = rv.lum(np.array([3, 3, 3], np.float32))
    n = np.float32(3)
    assert rec["rejected"] == 4 and rec["mixed"] == 1
    assert bits(var)[1] == 0 and bits(var)[3] == 0 and bits(frame)[3].tolist() == [0, 0, 0]
    s1 = (np.float32(0) + l1) + l3
    s2 = (np.float32(0) + l1 * l1) + l3 * l3
    mean = s1 / n
    v = s2 / n - mean * mean
    assert v > 0 and bits(var)[2] == bits(np.float32(v / np.float32(2)))
    assert bits(frame)[2].tolist() == bits((np.float32(0) + one + np.float32(3)) / n).repeat(3).tolist()
    assert var[0] >= 0 and var[0] <= np.float32(2.0 ** -22)   # a rounding residue at most


# ---- the rebuilt frame is the oracle's, on every case the GPU test uses ----------------------------
@pytest.mark.parametrize("name", sorted(rv.CASES))
def test_rebuilt_frame_is_the_oracles(name):
    img, var, rec = rv.reference(name)
    ref, cnt = rv.oracle_frame(name)
    assert np.array_equal(bits(img), bits(ref)), name
    assert rec["rejected"] == cnt["rejected"]
    _, w, h, spp, kw = rv.CASES[name]
    assert var.shape == (h, w) and var.dtype == np.float32
    assert np.isfinite(var).all() and (var >= 0).all() and not np.signbit(var).any()
    print(f"{name}: zero-variance pixels {(var == 0).sum()} of {var.size}, rejected {rec['rejected']}, "
          f"mixed {rec['mixed']}, clamped {rec['clamped']}, negative v {rec['negative']}")


def test_zero_and_positive_variance_in_one_frame():
    for name in ("gi", "direct", "mixed_lit", "spheres", "two_level", "whitted_lds_130", "whitted_bvh_64"):
        var = rv.reference(name)[1]
        assert (var == 0).sum() >= 10 and (var > 0).sum() >= 10, name


def test_rejecting_frames_mix_accepted_and_rejected_samples():
    for name in ("rejects_gi", "rejects_direct"):
        _, var, rec = rv.reference(name)
        assert rec["rejected"] > 1000 and rec["mixed"] >= 50, (name, rec)
        assert (var > 0).any()
    assert rv.reference("whitted_rejects_65")[2]["rejected"] > 0
    assert rv.reference("whitted_rejects_65")[2]["mixed"] > 0


def test_the_clamp():
    """v = s2 / n - mean * mean is a difference of two rounded values, so for a pixel whose samples
    are all equal it can come out below zero by a rounding residue: the clamp is reached on these
    inputs (constant pixels of the Normal frame and of Whitted frames at 65 and 130 samples)."""
    reached = {n: rv.reference(n)[2]["negative"] for n in sorted(rv.CASES)}
    print("pixels with v < 0 before the clamp:", {n: k for n, k in reached.items() if k})
    assert sum(reached.values()) > 0


def test_shard_leaves_other_rows_zero():
    img, var, _ = rv.reference("shard")
    rows = np.arange(12) % 3 == 1
    assert not bits(img)[~rows].any() and not bits(var)[~rows].any()
    assert (var[rows] > 0).any()


def test_window_edges_are_among_the_whitted_cases():
    assert sorted(rv.CASES[n][3] for n in rv.CASES if n.startswith("whitted_lds")) == [2, 64, 65, 130]
    assert sorted(rv.CASES[n][3] for n in rv.WHITTED_BVH) == [2, 64, 65, 130]


# ---- the quality conditions: the sample variance against the filter's own spatial estimate --------------
FILTER = dict(iterations=4, sigma_luminance=4.0, variance_radius=3, sigma_normal=0.5, sigma_depth=32.0, sigma_albedo=0.2)


@pytest.fixture(scope="module")
def cornell():
    """scenes.cornell(64, 48) under GI at 16 and 64 spp against 2048 spp, filtered with the spatial
    estimate and with the sample variance; the masks as tests/test_denoise_var_restatement.py builds them"""
    w, h = 64, 48
    s = scenes.cornell(w, h)
    ref, _ = pyoracle.render(s, w, h, 2048)
    emitting = np.array([s.desc.objects[i].light >= 0 for i in range(s.desc.n_objects)] + [True])   # [-1]: a miss
    everything = np.ones((h, w), bool)
    out = {}
    for spp in (16, 64):
        noisy, var, _ = rv.render(s, w, h, spp, integrator="gi")
        assert np.array_equal(bits(noisy), bits(pyoracle.render(s, w, h, spp)[0]))
        planes, _, per = ar.render(s, w, h, spp)
        obj = per["obj"]
        one = (obj == obj[:, :1]).all(axis=1) & ~emitting[obj[:, 0]]
        mask = np.zeros((h, w), bool)
        for n, (i, j) in enumerate(per["pix"]):
            mask[i, j] = one[n]

        def rmse(a, m):
            return float(np.sqrt(np.mean((a[m].astype(np.float64) - ref[m].astype(np.float64)) ** 2)))

        def ratios(img):
            return rmse(img, mask) / rmse(noisy, mask), rmse(img, everything) / rmse(noisy, everything)

        est_mean = float(dv.estimate(noisy, planes["object"], FILTER["variance_radius"]).mean())
        est = ratios(dv.denoise_var(noisy, planes, None, **FILTER)[0])
        smp = ratios(dv.denoise_var(noisy, planes, var, **FILTER)[0])
        print(f"{spp} spp, RMSE ratio one-object / all: spatial estimate {est[0]:.4f} / {est[1]:.4f}, "
              f"sample variance {smp[0]:.4f} / {smp[1]:.4f}; mean estimate {est_mean:.4g}, mean sample variance {var.mean():.4g}, "
              f"zero-variance pixels {(var == 0).sum()}, mask {mask.sum()}")
        out[spp] = dict(estimate=est, sample=smp, mask=mask)
    return out


def test_sample_variance_beats_the_estimate_at_64_spp(cornell):
    c = cornell[64]
    assert c["mask"].sum() >= 500
    assert c["sample"][0] < c["estimate"][0] and c["sample"][1] < c["estimate"][1]


def test_sample_variance_still_improves_the_whole_frame_at_64_spp(cornell):
    assert cornell[64]["sample"][1] < 1.0


def test_sample_variance_beats_the_estimate_on_one_object_pixels_at_16_spp(cornell):
    assert cornell[16]["sample"][0] < cornell[16]["estimate"][0]
