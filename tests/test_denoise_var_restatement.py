"""The variance-guided denoiser's cases, checked without a GPU on the restatement alone
(tests/denoise_var_restatement.py): the frames tests/test_gpu_denoise_var.py compares with the
device's really reach the situations that test relies on, the filter reduces to xrt_denoise's when
its luminance term is off, and as specified it improves a low-spp Cornell frame against a converged
one by more than the plain filter does."""
import ctypes as C

import numpy as np
import pytest

import aov_restatement as ar
import denoise_restatement as dr
import denoise_var_restatement as dv
import pyoracle
from xraytracer_amd import abi, scenes


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_abi_constants():
    assert abi.XRT_ABI_VERSION == 14
    assert C.sizeof(abi.XrtDenoiseVarParams) == 36 and C.sizeof(abi.XrtDenoiseStats) == 32
    assert abi.XRT_DENOISE_VAR_MAX_RADIUS == 3 and 0 <= abi.XRT_DENOISE_VAR_TILED_ITERATIONS <= abi.XRT_DENOISE_MAX_ITERATIONS
    assert [n for n, _ in abi.XrtDenoiseVarParams._fields_] == [
        "width", "height", "iterations", "sigma_luminance", "sigma_normal", "sigma_depth", "sigma_albedo", "variance_radius",
        "flags"]


def test_null_context_is_rejected_without_a_gpu():
    lib = abi.lib()
    p = abi.XrtDenoiseVarParams(4, 4, 1, 4.0, 1.0, 1.0, 1.0, 3, 0)
    buf = np.zeros((4, 4, 3), np.float32)
    var = np.zeros((4, 4), np.float32)
    assert lib.xrt_denoise_var(None, C.byref(p), buf.ctypes.data, var.ctypes.data, None, buf.ctypes.data, var.ctypes.data, None) == -1
    assert lib.xrt_denoise_var_device(None, C.byref(p), None, None, None, None, None, None, None) == -1
    assert lib.xrt_denoise_var(None, None, None, None, None, None, None, None) == -1


def test_the_cases_the_issue_names_are_there():
    for it in range(1, 7):
        for stem, radius in (("synthetic", 3), ("synthetic_r1", 1)):
            w, h, _, kind, kw = dv.CASES[f"{stem}_{it}"]
            assert (w, h, kind, kw["iterations"], kw["variance_radius"]) == (37, 29, None, it, radius)
    for n in ("1x1", "2x3", "5x1", "1x40", "200x3", "3x200", "130x70"):
        w, h, _, kind, _ = dv.CASES[n]
        assert f"{w}x{h}" == n and kind is None
    v = dv.inputs("supplied")[2]
    assert v.dtype == np.float32 and (v >= 0).all() and np.isfinite(v).all() and (v == 0).sum() >= 10 and (v > 0).sum() > v.size // 2
    assert dv.inputs("subnormal")[2].min() > 0


@pytest.mark.parametrize("name", sorted(dv.CASES))
def test_every_output_is_finite(name):
    out, var, rec = dv.reference(name)
    w, h = dv.CASES[name][:2]
    assert out.shape == (h, w, 3) and out.dtype == np.float32 and var.shape == (h, w) and var.dtype == np.float32
    assert np.isfinite(out).all() and np.isfinite(var).all() and (var >= 0).all()
    assert rec["taps"] > 0


def test_subnormal_weights_and_underflow():
    _, _, rec = dv.reference("subnormal")
    assert rec["e_88_104"] > 0 and rec["e_above_104"] > 0
    assert rec["subnormal"] > 0     # nonzero subnormal weights
    assert rec["underflow"] > 0     # expf(-e) == +0 for a finite e


def test_object_stop_zeroes_positive_weights():
    for name in ("synthetic_3", "130x70", "supplied"):
        assert dv.reference(name)[2]["stopped_positive"] > 0, name


def test_estimate_windows():
    for name in ("synthetic_3", "synthetic_r1_3", "130x70"):
        rec = dv.reference(name)[2]
        assert rec["est_border_cut"] > 0, name     # windows cut by the image border
        assert rec["est_object_cut"] > 0, name     # ... and by the object stop
        assert rec["est_min_n"] >= 1.0
    w, h, _, _, kw = dv.CASES["130x70"]
    assert dv.reference("130x70")[2]["est_border_cut"] < w * h    # and whole windows exist
    # pixels whose estimate is exactly 0: a one-pixel window, and pixels alone on their object in the window
    assert dv.reference("1x1")[2]["est_zero"] == 1
    color, g, _ = dv.inputs("synthetic_3")
    lone = np.array(g["object"])
    lone[10, 10] = 7
    rec = {}
    var = dv.estimate(color, lone, 3, rec)
    assert var[10, 10] == 0 and rec["est_zero"] >= 1 and bits(var)[10, 10] == 0


def test_iterations_and_radii_differ():
    outs = [dv.reference(n)[0] for n in dv.SYNTHETIC]
    for a, b in zip(outs, outs[1:]):
        assert not np.array_equal(bits(a), bits(b))
    assert not np.array_equal(bits(dv.reference("synthetic_3")[0]), bits(dv.reference("synthetic_r1_3")[0]))


@pytest.mark.parametrize("iterations", [1, 3, 6])
def test_luminance_off_is_the_plain_filter_with_colour_off(iterations):
    color, g, _ = dv.inputs("synthetic_3")
    sig = dict(sigma_normal=0.5, sigma_depth=1.0, sigma_albedo=0.2)
    want = dr.denoise(color, g, iterations=iterations, sigma_color=0.0, **sig)
    for off in (0.0, -1.0):
        got, var = dv.denoise_var(color, g, iterations=iterations, sigma_luminance=off, variance_radius=3, **sig)
        assert np.array_equal(bits(got), bits(want)), (iterations, off)
        assert np.isfinite(var).all() and (var >= 0).all()


def test_zero_variance_leaves_the_frame():
    """kl = 1 / 1e-8 everywhere: any tap whose luminance differs at all weighs at most expf(-dl 1e8)"""
    color, g, _ = dv.inputs("synthetic_3")
    zero = np.zeros(color.shape[:2], np.float32)
    out, var = dv.denoise_var(color, g, zero, **dv.CASES["synthetic_3"][4])
    assert np.abs(out - color).max() <= 2.0 ** -22 * np.abs(color).max()
    assert (var == 0).all()


def test_filtering_reduces_the_variance():
    color, g, _ = dv.inputs("synthetic_3")
    est = dv.estimate(color, g["object"], 3)
    assert dv.reference("synthetic_3")[1].mean() < est.mean()
    v = dv.inputs("supplied")[2]
    assert dv.reference("supplied")[1].mean() < v.mean()


# ---- the quality conditions: a 16 spp Cornell frame against a 2048 spp one ----------------------
@pytest.fixture(scope="module")
def cornell():
    """test_denoise_restatement.test_filter_improves_a_low_spp_cornell_frame's frame and masks"""
    w, h, spp = 64, 48, 16
    s = scenes.cornell(w, h)
    noisy, _ = pyoracle.render(s, w, h, spp)
    planes, _, per = ar.render(s, w, h, spp)
    ref, _ = pyoracle.render(s, w, h, 2048)
    obj = per["obj"]
    emitting = np.array([s.desc.objects[i].light >= 0 for i in range(s.desc.n_objects)] + [True])   # [-1]: a miss
    one = (obj == obj[:, :1]).all(axis=1) & ~emitting[obj[:, 0]]
    mask = np.zeros((h, w), bool)
    for n, (i, j) in enumerate(per["pix"]):
        mask[i, j] = one[n]
    everything = np.ones((h, w), bool)

    def rmse(a, m):
        return float(np.sqrt(np.mean((a[m].astype(np.float64) - ref[m].astype(np.float64)) ** 2)))

    def ratios(out):
        return rmse(out, mask) / rmse(noisy, mask), rmse(out, everything) / rmse(noisy, everything)

    guide = dict(sigma_normal=0.5, sigma_depth=32.0, sigma_albedo=0.2)
    plain = {it: ratios(dr.denoise(noisy, planes, iterations=it, sigma_color=2.0, **guide)) for it in (2, 3, 4, 5)}
    guided = {it: ratios(dv.denoise_var(noisy, planes, None, iterations=it, sigma_luminance=4.0, variance_radius=3, **guide)[0])
              for it in (3, 4, 5)}
    for it in sorted(plain):
        print(f"{it} iterations, RMSE ratio one-object / all: plain {plain[it][0]:.4f} / {plain[it][1]:.4f}"
              + (f", variance-guided {guided[it][0]:.4f} / {guided[it][1]:.4f}" if it in guided else ""))
    return dict(mask=mask, plain=plain, guided=guided)


def test_guided_filter_improves_a_low_spp_cornell_frame(cornell):
    assert cornell["mask"].sum() >= 1000
    assert cornell["guided"][4][0] <= 0.6


def test_guided_filter_beats_the_plain_filter_over_the_whole_frame(cornell):
    assert cornell["guided"][4][1] < cornell["plain"][2][1]


@pytest.mark.parametrize("iterations", [3, 4, 5])
def test_guided_filter_beats_the_plain_filter_at_the_same_count(cornell, iterations):
    assert cornell["guided"][iterations][0] < cornell["plain"][iterations][0]
