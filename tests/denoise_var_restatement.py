"""The variance-guided a-trous filter (xrt_denoise_var) restated in numpy — a test helper, not a
test file, in the style of tests/denoise_restatement.py, whose frames and helpers it reuses.

float32 throughout, one operation per statement, the loops of include/xrt.h vectorised per tap:
the estimate's (2 r + 1)^2 taps, the 3 x 3 variance prefilter's 9 and the filter's 25 are each
visited in the order dy outer, dx inner, and a tap updates exactly the pixels for which it lies
inside the image (and, for the estimate, on the centre's object), so every pixel sees its valid
taps in that order.  expf is the host glibc's; np.sqrt and / on float32 are correctly rounded.

CASES are the frames tests/test_gpu_denoise_var.py compares with the device's bit for bit, each
restated once per session (``reference``); tests/test_denoise_var_restatement.py checks without a
GPU that they reach the situations the GPU test relies on.
"""
import functools

import numpy as np

from denoise_restatement import F, H5, _d2, _window, expf, sigma_inv, synth

G3 = np.array([0.25, 0.5, 0.25], F)
DEFAULTS = dict(iterations=4, sigma_luminance=4.0, sigma_normal=0.5, sigma_depth=0.0, sigma_albedo=0.2, variance_radius=3)


def lum(c):
    r = F(0.2126) * c[..., 0]
    g = F(0.7152) * c[..., 1]
    b = F(0.0722) * c[..., 2]
    s = r + g
    return s + b


def estimate(color, obj, radius, record=None):
    """the (H, W) variance estimate of `color` over windows of (2 radius + 1)^2 pixels of the centre's object"""
    h, w = color.shape[:2]
    l = lum(np.asarray(color, F))
    n = np.zeros((h, w), F)
    m1 = np.zeros((h, w), F)
    m2 = np.zeros((h, w), F)
    inside = np.zeros((h, w), np.int64)
    for dy in range(-radius, radius + 1):
        wy = _window(h, dy)
        if wy is None:
            continue
        for dx in range(-radius, radius + 1):
            wx = _window(w, dx)
            if wx is None:
                continue
            p, q = (wy[0], wx[0]), (wy[1], wx[1])
            same = obj[p] == obj[q]
            lq = l[q]
            sq = lq * lq
            n[p] = np.where(same, n[p] + F(1.0), n[p])
            m1[p] = np.where(same, m1[p] + lq, m1[p])
            m2[p] = np.where(same, m2[p] + sq, m2[p])
            inside[p] += 1
    mean = m1 / n
    ex2 = m2 / n
    mm = mean * mean
    v = ex2 - mm
    var = np.where(v > 0, v, F(0.0)).astype(F)
    if record is not None:
        full = (2 * radius + 1) ** 2
        record.update(est_border_cut=int((inside < full).sum()), est_object_cut=int((n < inside).sum()),
                      est_zero=int((var == 0).sum()), est_min_n=float(n.min()))
    return var


def prefilter(var):
    """the 3 x 3 Gaussian of the variance plane at spacing 1, renormalised at the image border"""
    h, w = var.shape
    vs = np.zeros((h, w), F)
    gs = np.zeros((h, w), F)
    for dy in range(-1, 2):
        wy = _window(h, dy)
        if wy is None:
            continue
        for dx in range(-1, 2):
            wx = _window(w, dx)
            if wx is None:
                continue
            p, q = (wy[0], wx[0]), (wy[1], wx[1])
            gw = G3[dy + 1] * G3[dx + 1]
            t = var[q] * gw
            vs[p] = vs[p] + t
            gs[p] = gs[p] + gw
    return vs / gs


def denoise_var(color, guides=None, variance=None, iterations=4, sigma_luminance=4.0, sigma_normal=0.5, sigma_depth=0.0,
                sigma_albedo=0.2, variance_radius=3, record=None):
    """(the filtered (H, W, 3) frame, the (H, W) variance left), float32.  guides as for
    denoise_restatement.denoise; variance: (H, W) float32 or None (the estimate).
    record: a dict that receives tap counts (see test_denoise_var_restatement.py)."""
    g = guides or {}
    h, w = color.shape[:2]
    c = np.array(color, F)
    albedo = np.zeros((h, w, 3), F) if g.get("albedo") is None else g["albedo"]
    normal = np.zeros((h, w, 3), F) if g.get("normal") is None else g["normal"]
    depth = np.zeros((h, w), F) if g.get("depth") is None else g["depth"]
    obj = np.zeros((h, w), np.int32) if g.get("object") is None else g["object"]
    inv_n, inv_z, inv_a = (sigma_inv(s) for s in (sigma_normal, sigma_depth, sigma_albedo))
    sl = F(sigma_luminance)
    if record is not None:
        record.update(taps=0, subnormal=0, underflow=0, stopped_positive=0, e_88_104=0, e_above_104=0)
    var = np.array(variance, F) if variance is not None else estimate(c, obj, variance_radius, record)
    for i in range(iterations):
        s = 1 << i
        scale = F(1 << (2 * i))
        kz = inv_z * (F(1.0) / scale)
        kn, ka = inv_n, inv_a
        if sl > 0:
            vg = prefilter(var)
            sd = np.sqrt(vg)
            den = sl * sd
            den = den + F(1e-8)
            kl = F(1.0) / den
        else:
            kl = np.zeros((h, w), F)
        l = lum(c)
        acc = np.zeros((h, w, 3), F)
        vacc = np.zeros((h, w), F)
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
                dl = np.abs(l[p] - l[q])
                d2n = _d2(normal[p], normal[q])
                d2a = _d2(albedo[p], albedo[q])
                dz = depth[p] - depth[q]
                d2z = dz * dz
                tl = dl * kl[p]
                tn = d2n * kn
                tz = d2z * kz
                ta = d2a * ka
                e = tl + tn
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
                w2 = wt * wt
                tv = var[q] * w2
                vacc[p] = vacc[p] + tv
                ws[p] = ws[p] + wt
        c = acc / ws[..., None]
        ws2 = ws * ws
        var = vacc / ws2
    return c, var


# name -> (width, height, seed, variance kind, filter settings); variance kind None: the estimate
CASES = {}
_ON = dict(sigma_luminance=4.0, sigma_normal=0.5, sigma_depth=1.0, sigma_albedo=0.2)
# odd sizes, no tile multiple; at iteration 5 the taps reach 32 pixels, beyond the frame's height
for _it in range(1, 7):
    CASES[f"synthetic_{_it}"] = (37, 29, 11, None, dict(iterations=_it, variance_radius=3, **_ON))
    CASES[f"synthetic_r1_{_it}"] = (37, 29, 11, None, dict(iterations=_it, variance_radius=1, **_ON))
DEGENERATE = ("1x1", "2x3", "5x1", "1x40")
SEAMS = ("200x3", "3x200", "130x70")   # cross the seams of any tile up to 64 x 32
for _n in DEGENERATE + SEAMS:
    _w, _h = (int(v) for v in _n.split("x"))
    CASES[_n] = (_w, _h, 23, None, dict(iterations=3, variance_radius=2, **_ON))
# a caller's variance plane: positive, with some exact zeros (there kl = 1 / 1e-8 unless a neighbour's variance leaks in)
CASES["supplied"] = (37, 29, 17, "seeded", dict(iterations=3, variance_radius=3, **_ON))
# sqrt(var) in [1/91, 1/45] and sigma_luminance 0.9 give kl of 50 .. 100: luminance differences of
# 1 .. 2 put e in [88, 104) (subnormal expf), larger ones and the outliers above
CASES["subnormal"] = (37, 29, 31, "small", dict(iterations=2, variance_radius=3, sigma_luminance=0.9, sigma_normal=0.5,
                                                 sigma_depth=1.0, sigma_albedo=0.2))
SYNTHETIC = tuple(f"synthetic_{i}" for i in range(1, 7))


def supplied_variance(kind, w, h, seed):
    rng = np.random.default_rng(seed + 1000)
    u = rng.random((h, w), dtype=F)
    if kind == "seeded":
        v = (u * F(2.0)).astype(F)
        v[rng.random((h, w)) < 0.08] = F(0.0)
        return v
    assert kind == "small"
    return (F(1.0 / 8192.0) + u * F(3.0 / 8192.0)).astype(F)


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(color, guides, variance or None) of CASES[name]; read-only"""
    w, h, seed, kind, _ = CASES[name]
    color, guides = synth(w, h, seed)
    variance = None if kind is None else supplied_variance(kind, w, h, seed)
    for a in (color, variance) + tuple(guides.values()):
        if a is not None:
            a.setflags(write=False)
    return color, guides, variance


@functools.lru_cache(maxsize=None)
def reference(name):
    """(filtered frame, variance left, tap record) of the restatement for CASES[name]; computed once, read-only"""
    color, guides, variance = inputs(name)
    rec = {}
    out, var = denoise_var(color, guides, variance, record=rec, **CASES[name][4])
    out.setflags(write=False)
    var.setflags(write=False)
    return out, var, rec
