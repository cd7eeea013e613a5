"""The denoiser cases, checked without a GPU on the restatement alone
(tests/denoise_restatement.py): the frames tests/test_gpu_denoise.py compares with the device's
really reach the situations that test relies on, and the filter as specified improves a low-spp
Cornell frame against a converged one."""
import ctypes as C

import numpy as np
import pytest

import aov_restatement as ar
import denoise_restatement as dr
import pyoracle
from xraytracer_amd import abi, scenes


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_abi_constants():
    assert abi.XRT_ABI_VERSION == 14
    assert abi.XRT_DENOISE_MAX_ITERATIONS == 6 and 0 <= abi.XRT_DENOISE_TILED_ITERATIONS <= 6
    assert (abi.XRT_DENOISE_TIMING, abi.XRT_DENOISE_NO_TILE) == (1, 2)
    assert C.sizeof(abi.XrtDenoiseParams) == 32 and C.sizeof(abi.XrtDenoiseStats) == 32
    assert set(abi.DENOISE_PLANES) == set(dr.GUIDES) and set(dr.GUIDES) < set(abi.AOV_PLANES)


@pytest.mark.parametrize("name", sorted(dr.CASES))
def test_every_output_is_finite(name):
    out, rec = dr.reference(name)
    w, h, _, _ = dr.CASES[name]
    assert out.shape == (h, w, 3) and out.dtype == np.float32
    assert np.isfinite(out).all()
    assert rec["taps"] > 0


def test_case_inputs():
    color, g = dr.inputs("synthetic_3")
    assert color.min() >= 0 and (color == 25.0).sum() >= 3 and (color[color != 25.0] < 4).all()
    assert set(np.unique(g["object"])) == {-1, 0, 1}
    assert len(np.unique(g["normal"].reshape(-1, 3), axis=0)) == 3
    assert len(np.unique(g["albedo"].reshape(-1, 3), axis=0)) == 3
    assert np.abs(np.diff(g["depth"], axis=1)).max() > 3.0   # the step


def test_whole_tap_rows_fall_outside():
    """synthetic at 6 iterations: the last two spacings are 16 and 32, and 2 * 16 = 32 > 29 rows"""
    _, h, _, kw = dr.CASES["synthetic_6"]
    assert kw["iterations"] == 6 and 2 * 16 >= h and dr._window(h, 32) is None and dr._window(h, 16) is not None
    # so fewer taps were visited than 25 per pixel and iteration, in every case
    for name in dr.CASES:
        w, h, _, kw = dr.CASES[name]
        assert dr.reference(name)[1]["taps"] < 25 * w * h * kw["iterations"]


def test_subnormal_weights_and_underflow():
    _, rec = dr.reference("subnormal")
    assert rec["e_88_104"] > 0 and rec["e_above_104"] > 0
    assert rec["subnormal"] > 0     # nonzero subnormal weights
    assert rec["underflow"] > 0     # expf(-e) == +0 for a finite e


def test_object_stop_zeroes_positive_weights():
    for name in ("synthetic_3", "130x70", "subnormal"):
        assert dr.reference(name)[1]["stopped_positive"] > 0, name


def test_iterations_differ():
    outs = [dr.reference(n)[0] for n in dr.SYNTHETIC]
    for a, b in zip(outs, outs[1:]):
        assert not np.array_equal(bits(a), bits(b))


def test_null_plane_equals_zero_plane():
    color, g = dr.inputs("synthetic_2")
    kw = dr.CASES["synthetic_2"][3]
    h, w = color.shape[:2]
    zeros = dict(albedo=np.zeros((h, w, 3), np.float32), normal=np.zeros((h, w, 3), np.float32),
                 depth=np.zeros((h, w), np.float32), object=np.zeros((h, w), np.int32))
    for k in dr.GUIDES:
        without = {n: a for n, a in g.items() if n != k}
        assert np.array_equal(bits(dr.denoise(color, without, **kw)), bits(dr.denoise(color, dict(without, **{k: zeros[k]}), **kw)))
    assert np.array_equal(bits(dr.denoise(color, None, **kw)), bits(dr.denoise(color, zeros, **kw)))
    # and the planes matter: the full call differs from the bare one
    assert not np.array_equal(bits(dr.denoise(color, None, **kw)), bits(dr.reference("synthetic_2")[0]))


def test_sigma_off_equals_null_plane():
    color, g = dr.inputs("synthetic_2")
    kw = dr.CASES["synthetic_2"][3]
    for k, s in (("albedo", "sigma_albedo"), ("normal", "sigma_normal"), ("depth", "sigma_depth")):
        for off in (0.0, -1.0):
            a = dr.denoise(color, g, **dict(kw, **{s: off}))
            b = dr.denoise(color, {n: v for n, v in g.items() if n != k}, **kw)
            assert np.array_equal(bits(a), bits(b)), (k, off)


def test_one_by_one_frame_is_unchanged():
    color, _ = dr.inputs("1x1")
    out, _ = dr.reference("1x1")
    # one tap of weight 9/64: c * w / w, within an ulp of c
    assert np.abs(out - color).max() <= 2.0 ** -22 * np.abs(color).max()


def test_null_context_is_rejected_without_a_gpu():
    lib = abi.lib()
    p = abi.XrtDenoiseParams(4, 4, 1, 1.0, 1.0, 1.0, 1.0, 0)
    buf = np.zeros((4, 4, 3), np.float32)
    assert lib.xrt_denoise(None, C.byref(p), buf.ctypes.data, None, buf.ctypes.data, None) == -1
    assert lib.xrt_denoise_device(None, C.byref(p), None, None, None, None, None) == -1
    assert lib.xrt_denoise(None, None, None, None, None, None) == -1


# ---- the quality condition: a 16 spp Cornell frame against a 2048 spp one -----------------------
def test_filter_improves_a_low_spp_cornell_frame():
    """cornell(64, 48) under GI: the 16 spp frame, filtered with 2 iterations over the restated
    guide planes, against the 2048 spp frame.  Over the pixels whose 16 samples all hit one
    non-emitting object the RMSE must fall to at most 0.6 of the unfiltered frame's; over all
    pixels it must fall at all."""
    w, h, spp = 64, 48, 16
    s = scenes.cornell(w, h)
    noisy, _ = pyoracle.render(s, w, h, spp)
    planes, _, per = ar.render(s, w, h, spp)
    ref, _ = pyoracle.render(s, w, h, 2048)
    out = dr.denoise(noisy, planes, iterations=2, sigma_color=2.0, sigma_normal=0.5, sigma_depth=32.0, sigma_albedo=0.2)
    obj = per["obj"]
    emitting = np.array([s.desc.objects[i].light >= 0 for i in range(s.desc.n_objects)] + [True])   # [-1]: a miss
    one = (obj == obj[:, :1]).all(axis=1) & ~emitting[obj[:, 0]]
    mask = np.zeros((h, w), bool)
    for n, (i, j) in enumerate(per["pix"]):
        mask[i, j] = one[n]

    def rmse(a, m):
        return float(np.sqrt(np.mean((a[m].astype(np.float64) - ref[m].astype(np.float64)) ** 2)))

    everything = np.ones((h, w), bool)
    inner = rmse(out, mask) / rmse(noisy, mask)
    whole = rmse(out, everything) / rmse(noisy, everything)
    print(f"pixels on one non-emitting object: {int(mask.sum())} of {w * h}; RMSE ratio there {inner:.4f}, over all {whole:.4f}")
    assert mask.sum() >= 1000
    assert inner <= 0.6
    assert whole < 1.0
