"""WhittedIntegrator restated on the frozen oracle — a test helper, not a test file.

The reference's integrator.h, light.cpp and scene.* cannot be compiled here (spdlog, OpenCV,
tinyobjloader; oracle/Makefile:8-11), so the checker of XRT_INTEGRATOR_WHITTED is assembled
from three parts:

  a. this restatement of Src/integrator.h:303-393, Src/light.cpp:115-142 and
     Src/renderer.cpp:29-81, numpy float32 throughout, one operation per statement so the
     evaluation order is explicit.  It takes from oracle/pyoracle.py the per-pixel stream
     (``draws``, seed j + W*i), the camera ray (``orc_kat_camera``) and Scene::intersect /
     Scene::occluded (``orc_query``, the function ``pyoracle.query`` wraps, called here with
     numpy buffers so a whole queue level is one call);
  b. reflect / refract / fresnel / normalize / multVecMatrix / multDirMatrix below are pinned
     bit for bit to the reference's own geometry.cpp through tests/golden/ref_whitted_kats.json
     (tests/cpp/ref_whitted_kats.cpp is the driver that printed it);
  c. the queue logic itself is restated by reading: nothing compiled from the reference pins it.

The reference pops a std::queue and adds to total_radiance in pop order.  FIFO order is level
order (all rays of depth d before any of depth d + 1), and within a level the order the
parents pushed (glass: refracted first, then reflected).  ``render`` walks the queue level by
level for all samples of the frame at once and adds each sample's contributions in that order.

orc_query and directions (checked on the CPU, tests/test_whitted_restatement.py):
  * a non-unit direction is taken as given: t is the ray parameter, position = o + d * t;
  * a NaN direction hits nothing: every triangle test fails its final ``t > eps`` and a sphere
    reports a hit with t = NaN that no ``t < best`` accepts, so Scene::intersect returns true
    with hitObject null — undefined behaviour in the reference.  Here, and in the kernel,
    ``object < 0`` is a miss (the sky colour).
"""
import ctypes as C

import numpy as np

import pyoracle
from xraytracer_amd import abi

F = np.float32
SKY = (F(0.235294), F(0.67451), F(0.843137))   # Vec3f(0.235294, 0.67451, 0.843137)
IOR = F(1.3)
FLT_MAX = np.finfo(np.float32).max
HIT_WORDS = C.sizeof(abi.XrtHit) // 4


def _quiet():
    return np.errstate(all="ignore")


# ---------------------------------------------------------------- geometry.cpp / geometry.h
def dot(a, b):
    x = a[..., 0] * b[..., 0]
    y = a[..., 1] * b[..., 1]
    z = a[..., 2] * b[..., 2]
    s = x + y
    return s + z


def muls(v, k):
    """Vec3 * float (Src/geometry.h:212-215); k broadcasts per vector"""
    k = np.asarray(k, F)
    return v * k[..., None]


def divs(v, k):
    """Vec3 / float (Src/geometry.h:228-231)"""
    k = np.asarray(k, F)
    return v / k[..., None]


def length(v):
    return np.sqrt(dot(v, v))


def normalize(v):
    """Src/geometry.cpp:13-16: v / length(v)"""
    with _quiet():
        return divs(v, length(v))


def clamp(v, lo, hi):
    """std::clamp: (v < lo) ? lo : (hi < v) ? hi : v"""
    return np.where(v < lo, lo, np.where(hi < v, hi, v)).astype(F)


def smax(a, b):
    """std::max(a, b): (a < b) ? b : a"""
    return np.where(a < b, b, a).astype(F)


def reflect(I, N):
    """Src/geometry.cpp:52-55: I - 2 * dot(I, N) * N"""
    k = F(2.0) * dot(I, N)
    t = muls(N, k)
    return I - t


def refract(I, N, ior=IOR):
    """Src/geometry.cpp:57-67"""
    with _quiet():
        cosi = clamp(dot(I, N), F(-1.0), F(1.0))
        neg = cosi < F(0.0)
        cosi = np.where(neg, -cosi, cosi).astype(F)
        etai = np.where(neg, F(1.0), ior).astype(F)
        etat = np.where(neg, ior, F(1.0)).astype(F)
        n = np.where(neg[..., None], N, -N).astype(F)
        eta = etai / etat
        e2 = eta * eta
        c2 = cosi * cosi
        om = F(1.0) - c2
        p = e2 * om
        k = F(1.0) - p
        a = muls(I, eta)
        ec = eta * cosi
        sq = np.sqrt(k)
        b = muls(n, ec - sq)
        r = a + b
        return np.where((k < F(0.0))[..., None], F(0.0), r).astype(F)


def fresnel(I, N, ior=IOR):
    """Src/geometry.cpp:69-89: kr"""
    with _quiet():
        cosi = clamp(dot(I, N), F(-1.0), F(1.0))
        pos = cosi > F(0.0)
        etai = np.where(pos, ior, F(1.0)).astype(F)
        etat = np.where(pos, F(1.0), ior).astype(F)
        q = etai / etat
        c2 = cosi * cosi
        om = F(1.0) - c2
        sint = q * np.sqrt(smax(F(0.0), om))
        s2 = sint * sint
        cost = np.sqrt(smax(F(0.0), F(1.0) - s2))
        ca = np.abs(cosi)
        tc = etat * ca
        ic = etai * cost
        Rs = (tc - ic) / (tc + ic)
        ia = etai * ca
        tt = etat * cost
        Rp = (ia - tt) / (ia + tt)
        rs2 = Rs * Rs
        rp2 = Rp * Rp
        kr = (rs2 + rp2) / F(2.0)
        return np.where(sint >= F(1.0), F(1.0), kr).astype(F)


def mult_vec_matrix(src, m):
    """Matrix44::multVecMatrix (Src/geometry.h:466-478); m row-major (16,)"""
    x = np.asarray(m, F).reshape(4, 4)
    s = np.asarray(src, F)
    out = []
    for c in range(4):
        t = s[0] * x[0][c]
        t = t + s[1] * x[1][c]
        t = t + s[2] * x[2][c]
        t = t + x[3][c]
        out.append(F(t))
    with _quiet():
        return np.array([out[0] / out[3], out[1] / out[3], out[2] / out[3]], F)


def mult_dir_matrix(src, m):
    """Matrix44::multDirMatrix (Src/geometry.h:487-498)"""
    x = np.asarray(m, F).reshape(4, 4)
    s = np.asarray(src, F)
    out = []
    for c in range(3):
        t = s[0] * x[0][c]
        t = t + s[1] * x[1][c]
        t = t + s[2] * x[2][c]
        out.append(F(t))
    return np.array(out, F)


def point_light_pos(l2w):
    """PointLight::PointLight (Src/light.cpp:115-118)"""
    return mult_vec_matrix((0.0, 0.0, 0.0), l2w)


def distant_light_dir(l2w):
    """DistantLight::DistantLight (Src/light.cpp:130-134)"""
    return normalize(mult_dir_matrix((0.0, 0.0, -1.0), l2w))


# ---------------------------------------------------------------- Scene::intersect / occluded
def _query(scene, o, d, tmax=None):
    """orc_query over rays (o, d) [n, 3]: the hit records as an [n, HIT_WORDS] float32 array
    (view the first three columns as int32: hit, object, primitive)"""
    n = len(o)
    rays = np.ascontiguousarray(np.concatenate([o, d], axis=1), dtype=F)
    out = np.zeros((max(1, n), HIT_WORDS), F)
    tm = None if tmax is None else np.ascontiguousarray(tmax, dtype=F)
    rc = pyoracle.lib().orc_query(C.byref(scene.desc), n, pyoracle.fp(rays), pyoracle.fp(tm) if tm is not None else None,
                                  1 if tmax is not None else 0, out.ctypes.data_as(C.POINTER(abi.XrtHit)))
    assert rc == 0
    return out[:n]


def intersect(scene, o, d):
    """Scene::intersect on fresh IntersectInfos: (object [n] int, position, ng, ns [n, 3])"""
    h = _query(scene, o, d)
    obj = h[:, 1].view(np.int32).copy()
    return obj, h[:, 5:8].copy(), h[:, 8:11].copy(), h[:, 11:14].copy()


def occluded(scene, o, d, tmax):
    return _query(scene, o, d, tmax)[:, 0].view(np.int32) != 0


def delta_lights(scene):
    p, n = scene.delta_lights()
    return [(int(p[i].kind), np.array(p[i].pos[:], F), np.array(p[i].dir[:], F), np.array(p[i].color[:], F),
             F(p[i].intensity)) for i in range(n)]


# ---------------------------------------------------------------- WhittedIntegrator::integrate
def integrate(scene, ro, rd, max_depth, lights=None):
    """Src/integrator.h:303-393 for camera rays (ro, rd) [S, 3].  Returns (radiance [S, 3],
    counters dict, per-sample dict of arrays: cut (depth-overflow pops), rays (pops),
    shadow (occluded calls), shadow_hit (of them occluded), first_obj (the camera ray's
    hitObject, -1 none), radiance (what integrate returned))."""
    S = len(ro)
    lights = delta_lights(scene) if lights is None else lights
    mats = np.array([scene.desc.objects[i].material for i in range(scene.desc.n_objects)] + [abi.XRT_MAT_NONE], np.int32)
    albedo = np.array([scene.desc.objects[i].albedo[:] for i in range(scene.desc.n_objects)] + [(0, 0, 0)], F)
    sky = np.array(SKY, F)
    total = np.zeros((S, 3), F)
    cnt = dict(segments=0, shadow_rays=0, whit_rays=0, whit_depth_cut=0, whit_refract=0, whit_tir=0)
    per = dict(cut=np.zeros(S, np.int64), rays=np.zeros(S, np.int64), shadow=np.zeros(S, np.int64),
               shadow_hit=np.zeros(S, np.int64), first_obj=np.full(S, -1, np.int64))

    def add_in_order(sid, val):
        """total[sid] += val, one entry after the other in array order"""
        if len(sid) == 0:
            return
        first = np.r_[True, sid[1:] != sid[:-1]]
        start = np.maximum.accumulate(np.where(first, np.arange(len(sid)), 0))
        rank = np.arange(len(sid)) - start
        for r in range(int(rank.max()) + 1):
            m = rank == r
            with _quiet():
                total[sid[m]] = total[sid[m]] + val[m]

    sid = np.arange(S)
    o, d = np.asarray(ro, F).copy(), np.asarray(rd, F).copy()
    thr = np.ones((S, 3), F)   # ray_root.throughput = Vec3f(1, 1, 1), depth 0
    depth = 0
    with _quiet():
        while len(sid):
            n = len(sid)
            cnt["whit_rays"] += n
            np.add.at(per["rays"], sid, 1)
            if depth > max_depth:   # total_radiance += ray.throughput * sky; continue
                cnt["whit_depth_cut"] += n
                np.add.at(per["cut"], sid, 1)
                add_in_order(sid, thr * sky)
                break   # such rays push nothing: the queue is empty after this level
            obj, pos, ng, ns = intersect(scene, o, d)
            cnt["segments"] += n
            if depth == 0:
                per["first_obj"][sid] = obj
            mat = mats[obj]   # obj -1 -> the appended NONE entry (unused: misses add the sky)
            miss = obj < 0
            lam = ~miss & (mat == abi.XRT_MAT_LAMBERT)
            metal = ~miss & (mat == abi.XRT_MAT_METAL)
            glass = ~miss & (mat == abi.XRT_MAT_GLASS)
            contrib = np.zeros((n, 3), F)
            contrib[miss] = (thr * sky)[miss]
            if lam.any():
                li = np.nonzero(lam)[0]
                p, g, s = pos[li], ng[li], ns[li]
                rad = np.zeros((len(li), 3), F)
                fr = albedo[obj[li]] / F(3.14159265359)   # Lambert::evaluateBxDF = albedo / PI
                so = p + muls(g, F(0.1))   # position + ng * 0.1
                for kind, lpos, ldir, color, intensity in lights:
                    if kind == abi.XRT_DLIGHT_POINT:   # PointLight::sample
                        ld = lpos[None, :] - p
                        dist = length(ld)
                        wi = divs(ld, dist)
                        pdf = dist * dist
                        tmax = dist
                    else:   # DistantLight::sample
                        wi = np.broadcast_to(-ldir, p.shape).astype(F)
                        pdf = np.ones(len(li), F)
                        tmax = np.full(len(li), FLT_MAX, F)
                    L = muls(color, intensity)   # color * intensity
                    occ = occluded(scene, so, wi, tmax)
                    cnt["shadow_rays"] += len(li)
                    np.add.at(per["shadow"], sid[li], 1)
                    np.add.at(per["shadow_hit"], sid[li], occ.astype(np.int64))
                    vis = (~occ).astype(F)
                    t = muls(fr, vis)            # vis * fr
                    t = t * L[None, :]           # * light_L
                    c = smax(F(0.0), dot(s, wi))
                    t = muls(t, c)               # * std::max(0.f, dot(ns, wi))
                    t = divs(t, pdf)             # / pdf
                    rad = rad + t
                rad = rad * thr[li]              # radiance *= ray.throughput
                contrib[li] = rad
            adds = miss | lam
            add_in_order(sid[adds], contrib[adds])
            # children, in push order: slot 2i = the refracted ray of parent i, 2i + 1 = the reflected
            slot, c_sid, c_o, c_d, c_thr = [], [], [], [], []
            if metal.any():
                mi = np.nonzero(metal)[0]
                slot.append(2 * mi + 1)
                c_sid.append(sid[mi])
                c_o.append(pos[mi] + muls(ng[mi], F(0.001)))
                c_d.append(reflect(d[mi], ng[mi]))           # not normalised
                c_thr.append(muls(thr[mi], F(0.8)))
            if glass.any():
                gi = np.nonzero(glass)[0]
                I, N, p = d[gi], ng[gi], pos[gi]
                kr = fresnel(I, N)
                outside = dot(I, N) < F(0.0)
                bias = muls(N, F(0.001))
                t9 = muls(thr[gi], F(0.9))
                rf = kr < F(1.0)
                cnt["whit_refract"] += int(rf.sum())
                cnt["whit_tir"] += int((~rf).sum())
                om = F(1.0) - kr
                slot.append(2 * gi[rf])
                c_sid.append(sid[gi][rf])
                c_o.append(np.where(outside[:, None], p - bias, p + bias).astype(F)[rf])
                c_d.append(normalize(refract(I, N))[rf])
                c_thr.append(muls(t9, om)[rf])
                slot.append(2 * gi + 1)
                c_sid.append(sid[gi])
                c_o.append(np.where(outside[:, None], p + bias, p - bias).astype(F))
                c_d.append(normalize(reflect(I, N)))
                c_thr.append(muls(t9, kr))
            if not slot:
                break
            order = np.argsort(np.concatenate(slot), kind="stable")
            sid = np.concatenate(c_sid)[order]
            o = np.concatenate(c_o)[order]
            d = np.concatenate(c_d)[order]
            thr = np.concatenate(c_thr)[order]
            depth += 1
    per["radiance"] = total
    return total, cnt, per


# ---------------------------------------------------------------- NormalRenderer::render
def render(scene, width, height, spp, max_depth=None, shard_index=0, shard_count=1, initial=None):
    """Src/renderer.cpp:29-81 over the rows y % shard_count == shard_index with the Whitted
    integrator: returns ((H, W, 3) float32, counters dict, per-sample dict)."""
    max_depth = scene.max_depth if max_depth is None else max_depth
    cam = pyoracle.camera(scene.camera)
    rows = [i for i in range(height) if i % shard_count == shard_index]
    pix = [(i, j) for i in rows for j in range(width)]
    ro = np.zeros((len(pix), spp, 3), F)
    rd = np.zeros((len(pix), spp, 3), F)
    co, cd = np.zeros(3, F), np.zeros(3, F)
    lib = pyoracle.lib()
    for n, (i, j) in enumerate(pix):
        w = pyoracle.draws(j + width * i, 2 * spp)   # sampler_per_pixel->setSeed(j + width * i)
        for k in range(spp):
            u = F(F(j) + w[2 * k]) / F(width)
            v = F(F(i) + w[2 * k + 1]) / F(height)
            lib.orc_kat_camera(C.byref(cam), C.c_float(u), C.c_float(v), pyoracle.fp(co), pyoracle.fp(cd))
            ro[n, k], rd[n, k] = co, cd
    rad, cnt, per = integrate(scene, ro.reshape(-1, 3), rd.reshape(-1, 3), max_depth)
    with _quiet():
        rad = (rad / F(1.0)).reshape(len(pix), spp, 3)   # integrate(...) / pdf, pinhole pdf 1
    bad = np.isnan(rad).any(-1) | np.isinf(rad).any(-1) | (rad < 0).any(-1)
    img = np.zeros((height, width, 3), F)
    if initial is not None:
        img[...] = initial
    acc = np.array([img[i, j] for i, j in pix], F).reshape(len(pix), 3)
    for k in range(spp):   # Image::addPixel in sample order
        ok = ~bad[:, k]
        acc[ok] = acc[ok] + rad[ok, k]
    acc = acc / F(spp)     # image /= Vec3f(n_samples)
    for n, (i, j) in enumerate(pix):
        img[i, j] = acc[n]
    cnt.update(samples=len(pix) * spp, draws=2 * len(pix) * spp, rejected=int(bad.sum()),
               rng_twists=len(pix) * ((2 * spp + 623) // 624))
    per = {k: v.reshape((len(pix), spp) + v.shape[1:]) for k, v in per.items()}
    return img, cnt, per
