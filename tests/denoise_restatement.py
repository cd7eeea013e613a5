"""The edge-avoiding a-trous filter (xrt_denoise) restated in numpy — a test helper, not a test
file, in the style of tests/aov_restatement.py.

float32 throughout, one operation per statement, the loop of include/xrt.h vectorised per tap:
for each iteration the 25 taps are visited in the order dy outer, dx inner, and a tap updates
exactly the pixels for which it lies inside the image, so every pixel sees its valid taps in
that order.  expf is the host glibc's (``pyoracle.libm_logexpf``), not np.exp.

CASES are the frames tests/test_gpu_denoise.py compares with the device's bit for bit, each
restated once per session (``reference``); tests/test_denoise_restatement.py checks without a
GPU that they reach the situations the GPU test relies on.
"""
import functools

import numpy as np

import pyoracle

F = np.float32
H5 = np.array([1.0 / 16.0, 1.0 / 4.0, 3.0 / 8.0, 1.0 / 4.0, 1.0 / 16.0], F)
GUIDES = ("albedo", "normal", "depth", "object")
DEFAULTS = dict(iterations=3, sigma_color=2.0, sigma_normal=0.5, sigma_depth=0.0, sigma_albedo=0.2)


def sigma_inv(sigma):
    s = F(sigma)
    return F(1.0) / (s * s) if s > 0 else F(0.0)


def expf(x):
    return pyoracle.libm_logexpf(x.reshape(-1))[1].reshape(x.shape)


def _d2(p, q):
    d = p - q
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    xx = dx * dx
    yy = dy * dy
    zz = dz * dz
    s = xx + yy
    return s + zz


def _window(n, off):
    """(slice of centres p, slice of taps q = p + off) along an axis of length n; None if empty"""
    lo, hi = max(0, -off), min(n, n - off)
    return (slice(lo, hi), slice(lo + off, hi + off)) if lo < hi else None


def denoise(color, guides=None, iterations=3, sigma_color=2.0, sigma_normal=0.5, sigma_depth=0.0, sigma_albedo=0.2,
            record=None):
    """the filtered (H, W, 3) float32 frame.  guides: dict of albedo / normal (H, W, 3), depth
    (H, W) float32, object (H, W) int32; a missing or None plane is a plane of zeros.
    record: a dict that receives tap counts (see test_denoise_restatement.py)."""
    g = guides or {}
    h, w = color.shape[:2]
    c = np.array(color, F)
    albedo = np.zeros((h, w, 3), F) if g.get("albedo") is None else g["albedo"]
    normal = np.zeros((h, w, 3), F) if g.get("normal") is None else g["normal"]
    depth = np.zeros((h, w), F) if g.get("depth") is None else g["depth"]
    obj = np.zeros((h, w), np.int32) if g.get("object") is None else g["object"]
    inv_c, inv_n, inv_z, inv_a = (sigma_inv(s) for s in (sigma_color, sigma_normal, sigma_depth, sigma_albedo))
    if record is not None:
        record.update(taps=0, subnormal=0, underflow=0, stopped_positive=0, e_88_104=0, e_above_104=0)
    for i in range(iterations):
        s = 1 << i
        scale = F(1 << (2 * i))
        kc = inv_c * scale
        kz = inv_z * (F(1.0) / scale)
        kn, ka = inv_n, inv_a
        acc = np.zeros((h, w, 3), F)
        ws = np.zeros((h, w), F)
        for dy in range(-2, 3):
            wy = _window(h, s * dy)
            if wy is None:
                continue
            for dx in range(-2, 3):
                wx = _window(w, s * dx)
                if wx is None:
                    continue
                p, q = (wy[0], wx[0]), (wy[1], wx[1])
                d2c = _d2(c[p], c[q])
                d2n = _d2(normal[p], normal[q])
                d2a = _d2(albedo[p], albedo[q])
                dz = depth[p] - depth[q]
                d2z = dz * dz
                tc = d2c * kc
                tn = d2n * kn
                tz = d2z * kz
                ta = d2a * ka
                e = tc + tn
                e = e + tz
                e = e + ta
                ex = expf(-e)
                hw = H5[dy + 2] * H5[dx + 2]
                wt = ex * hw
                other = obj[p] != obj[q]
                if record is not None:
                    tiny = np.finfo(F).tiny
                    record["taps"] += wt.size
                    record["subnormal"] += int(((wt > 0) & (wt < tiny) & ~other).sum())
                    record["underflow"] += int(((ex == 0) & np.isfinite(e) & ~other).sum())
                    record["stopped_positive"] += int((other & (ex > 0)).sum())
                    record["e_88_104"] += int(((e >= 88) & (e <= F(103.9))).sum())
                    record["e_above_104"] += int((e > 104).sum())
                wt = np.where(other, F(0.0), wt)
                cq = c[q]
                acc[p] = acc[p] + cq * wt[..., None]
                ws[p] = ws[p] + wt
        c = acc / ws[..., None]
    return c


def synth(w, h, seed):
    """a seeded frame and its guide planes: colour uniform in [0, 4) with a handful of 25.0
    outliers, normals from three unit vectors by region, a depth ramp with a step, three albedo
    values, object ids -1, 0, 1 by region"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:h, 0:w]
    color = (rng.random((h, w, 3), dtype=F) * F(4.0)).astype(F)
    for _ in range(max(1, (w * h) // 200)):
        color[rng.integers(h), rng.integers(w), rng.integers(3)] = F(25.0)
    region = ((3 * x) // w + (2 * y) // h) % 3
    normal = np.array([(0.0, 0.0, 1.0), (0.0, 1.0, 0.0), (0.6, 0.8, 0.0)], F)[region]
    albedo = np.array([(0.8, 0.8, 0.8), (0.7, 0.2, 0.2), (0.2, 0.7, 0.2)], F)[((x + 2 * y) // 7) % 3]
    depth = (F(5.0) + F(0.05) * x.astype(F) + F(0.02) * y.astype(F) + F(3.0) * (x >= w // 2)).astype(F)
    obj = (region - 1).astype(np.int32)
    return color, dict(albedo=np.ascontiguousarray(albedo), normal=np.ascontiguousarray(normal), depth=depth, object=obj)


# name -> (width, height, seed, filter settings)
CASES = {}
# sigma_color 32: the colour factor is 4^i / 1024, so it still passes neighbours of this noise at the sixth iteration
_ON = dict(sigma_color=32.0, sigma_normal=0.5, sigma_depth=1.0, sigma_albedo=0.2)
# odd sizes, no tile multiple; at iteration 5 the taps reach 32 pixels, beyond the frame's height
for _it in range(1, 7):
    CASES[f"synthetic_{_it}"] = (37, 29, 11, dict(iterations=_it, **_ON))
DEGENERATE = ("1x1", "2x3", "5x1", "1x40")
SEAMS = ("200x3", "3x200", "130x70")   # cross the seams of any tile up to 64 x 32
for _n in DEGENERATE + SEAMS:
    _w, _h = (int(v) for v in _n.split("x"))
    CASES[_n] = (_w, _h, 23, dict(iterations=3, **_ON))
# colour distances of 5.5 .. 6.5 at kc = 16 give e in [88, 104): subnormal expf; the outliers go far above
CASES["subnormal"] = (37, 29, 31, dict(iterations=2, sigma_color=0.25, sigma_normal=0.5, sigma_depth=1.0, sigma_albedo=0.2))
SYNTHETIC = tuple(f"synthetic_{i}" for i in range(1, 7))


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(color, guides) of CASES[name]; read-only"""
    w, h, seed, _ = CASES[name]
    color, guides = synth(w, h, seed)
    color.setflags(write=False)
    for a in guides.values():
        a.setflags(write=False)
    return color, guides


@functools.lru_cache(maxsize=None)
def reference(name):
    """(filtered frame, tap record) of the restatement for CASES[name]; computed once, read-only"""
    color, guides = inputs(name)
    rec = {}
    out = denoise(color, guides, record=rec, **CASES[name][3])
    out.setflags(write=False)
    return out, rec
