"""What the GPU test modules (tests/test_gpu_*.py) share, each thing once: paths and the
examples' binaries, bit comparison of arrays, the comparison of a rendered frame, path counters
against the oracle's, and the render-and-compare helpers over HipRenderer.  The comparison
helpers need no GPU; tests/test_checks.py checks them on arrays of a few pixels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import pyoracle
import whitted_scenes as ws
from xraytracer_amd import abi
from xraytracer_amd.renderer import HipRenderer

# ------------------------------------------------------------------ paths and examples ----
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA_DIR = os.path.join(ROOT, "xraytracer_amd", "data") + os.sep   # what the examples take as XRT_DATA_DIR


def run_example(name, *args, env=None):
    """run examples/bin/<name> with the arguments (each through str) and return its stdout;
    env: variables set on top of this process's environment"""
    return subprocess.run([os.path.join(ROOT, "examples", "bin", name)] + [str(a) for a in args], check=True,
                          capture_output=True, text=True, env=None if env is None else dict(os.environ, **env)).stdout


def read_ppm(path, w, h):
    """the (h, w, 3) int64 values of a P3 PPM of that size and maxval 255"""
    with open(path) as f:
        tok = f.read().split()
    assert tok[:4] == ["P3", str(w), str(h), "255"], tok[:4]
    return np.array(tok[4:], np.int64).reshape(h, w, 3)


# ------------------------------------------------------------------ bits ----
def words(a):
    """the uint32 words of a float32 array; of an integer plane, those of its values as int32"""
    a = np.ascontiguousarray(a)
    if a.dtype == np.float32:
        return a.view(np.uint32)
    if a.dtype.kind not in "iu":
        raise TypeError(f"words() takes float32 or integer arrays, not {a.dtype}")
    return a.astype(np.int32).view(np.uint32)


def first_diff(a, b, n=4):
    """the first n elements whose words differ, as (index, a's value, b's value)"""
    d = np.argwhere(words(a) != words(b))
    return [(tuple(int(x) for x in q), a[tuple(q)].item(), b[tuple(q)].item()) for q in d[:n]]


def assert_same_bits(got, ref, what=""):
    """equal shape, dtype and words; the values may be any bits (NaN and inf included).
    what: a name for the message, such as the plane's"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert got.dtype == ref.dtype, (what, got.dtype, ref.dtype)
    n = int(np.count_nonzero(words(got) != words(ref)))
    assert n == 0, (what, n, first_diff(got, ref))


# ------------------------------------------------------------------ frames ----
RMSE_TOL = 1e-3  # BASELINE.json north_star: per-channel RMSE < 1e-3 at matched seeds; reported, not the bar


def assert_frame(img, ref):
    """The comparison of a rendered frame with the oracle's or a restatement's: equal shape, every
    value on both sides finite, equal bits — the sign of a zero included.  Finite and bit-equal
    frames have RMSE 0, so the north-star tolerance only appears in the message."""
    assert img.shape == ref.shape, (img.shape, ref.shape)
    assert np.all(np.isfinite(img)), np.argwhere(~np.isfinite(img))[:5]
    assert np.all(np.isfinite(ref)), np.argwhere(~np.isfinite(ref))[:5]
    assert img.dtype == ref.dtype, (img.dtype, ref.dtype)
    bad = np.argwhere(np.any(words(img) != words(ref), axis=-1))
    if len(bad):
        rmse = np.sqrt(np.mean((img.astype(np.float64) - ref.astype(np.float64)) ** 2, axis=tuple(range(img.ndim - 1))))
        first = [(tuple(int(x) for x in q), img[tuple(q)].tolist(), ref[tuple(q)].tolist()) for q in bad[:5]]
        raise AssertionError(f"{len(bad)} pixels differ; first (pixel, got, ref): {first}; "
                             f"per-channel RMSE {rmse.tolist()} (north star: < {RMSE_TOL})")


# ------------------------------------------------------------------ counters ----
COUNTERS = ("segments", "shadow_rays", "draws", "rejected", "stalled")


def counters_equal(g, st, names=COUNTERS):
    """the named xrt_stats fields of g equal the oracle's dictionary st"""
    for k in names:
        assert getattr(g, k) == st[k], (k, getattr(g, k), st[k])


# ------------------------------------------------------------------ rendering ----
@pytest.fixture(scope="module")
def renderer():
    r = HipRenderer(1, device=0)
    yield r
    r.close()


ORACLE_KW = ("integrator", "max_depth", "shard_index", "shard_count", "initial")   # what pyoracle.render takes


def render_pair(r, scene, w, h, spp, ref=None, **kw):
    """(the device's frame, the oracle's frame, the oracle's counters, the device's xrt_stats) of
    one scene at spp samples after a fresh upload.  kw goes to HipRenderer.render, and of it to
    the oracle what is semantics (ORACLE_KW), not launch geometry.  ref: the oracle's (image,
    stats) pair where it was computed before."""
    r.spp = spp
    r._uploaded = None
    img = r.render(scene, w, h, **kw)
    g = r.stats
    if ref is None:
        ref = pyoracle.render(scene, w, h, spp, **{k: v for k, v in kw.items() if k in ORACLE_KW})
    return img, ref[0], ref[1], g


def render_rc(scene, w, h, spp, **kw):
    """xrt_render's status and message for a render that may be refused"""
    r = HipRenderer(spp)
    try:
        r.upload(scene)
        p = r.params(scene, w, h, **kw)
        img = np.zeros((h, w, 3), np.float32)
        st = abi.XrtStats()
        rc = abi.lib().xrt_render(r.ctx, C.byref(p), abi.fptr(img), C.byref(st))
        return rc, abi.lib().xrt_last_error(r.ctx).decode()
    finally:
        r.close()


def check_whitted_case(cases, name, schedule, devices=None, **render_kw):
    """render cases.CASES[name] (cases: whitted_scenes or whitted_bvh_scenes) on the GPU and compare
    frame, counters and schedule with the restatement"""
    _, w, h, spp, depth, kw = cases.CASES[name]
    kw = dict(kw)
    initial = ws.initial_image(w, h) if kw.pop("initial", False) else None
    ref, cnt, per = cases.reference(name)
    r = HipRenderer(spp, devices=devices)
    try:
        img = r.render(cases.scene(name), w, h, initial=initial, max_depth=depth, **render_kw, **kw)
        st = r.stats
        assert st.schedule == schedule
        got = {k: int(getattr(st, k)) for k in ws.COUNTERS}
        assert got == {k: int(cnt[k]) for k in ws.COUNTERS}
        assert_frame(img, ref)
    finally:
        r.close()
    return img, cnt, per
