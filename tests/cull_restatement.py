"""The trace kernels' culls restated in numpy float32 — a test helper, not a test file, in the style
of tests/camlist_restatement.py.  It shares no code with the library.

Every trace kernel skips work the reference's in-order `t < best` scan would have done, and each
skip is claimed conservative.  What is restated here, from xraytracer_amd/csrc:

  Bounds::pad (api_scene.cpp)        pad(k) = k * diagonal + k of the boxes the structure is built
                                     over; k = 1e-3 for object boxes, 1e-4 for both BVHs
  build_small_scene (api_scene.cpp)  triangle scenes of at most 1024 triangles and 256 objects: one
                                     box per object over its triangles' boxes (v0, v0 + e1, v0 + e2
                                     in float), padded by pad(1e-3) of all of them
  build_tri_bvh (api_scene.cpp)      larger triangle scenes: objects of more than 256 triangles go
                                     into the BVH, the others (when they fit the small-scene limits)
                                     get padded object boxes as above — both pads from the bounds of
                                     the BVH's and the small objects' triangles together; triangles
                                     with an exactly zero edge vector are left out of the BVH
  per-triangle padded box            host/bvh.cpp set_child: a child's box is the union of its
                                     triangles' boxes (Builder::bounds) minus / plus the margin, at
                                     every level; a union's min is at most each member's and float
                                     subtraction is monotonic, so the triangle's own box padded by
                                     the margin lies inside the box of every node above it.  A ray
                                     that overlaps the triangle's padded box overlaps all of them:
                                     this is the strictest of the walk's tests, and the one restated.
  build_sphere_bvh (api_scene.cpp)   sphere scenes of at least 16 spheres: boxes centre -+ |r| in
                                     float, padded by pad(1e-4); the per-sphere padded box is
                                     restated for the same reason
  box_overlap (path_common.h), bvh_box (lscene.h)
                                     (b - o) * inv per slab, fminf / fmaxf, !(tn > tf)
  bvh_enter (path_common.h)          the same arithmetic; tn > tf ? inf : tn, and the walk enters
                                     when the result is not inf
  obj_overlap, box_overlap_f (merged.h)
                                     inv clamped to +-1e30, oi = o * inv, one fma(b, inv, -oi) per slab
  plane_tri_ok (api_scene.cpp), plane_away (merged.h), plane_away_w (bvh_walk.h)
                                     the plane an object lies in, and (o_a - c) * d_a >= 0

The device's reciprocal is v_rcp_f32, accurate to 1 ulp: every slab test is evaluated with the
correctly rounded float reciprocal and with its two float neighbours (`rcp_variants`), and a hit
counts as kept only if all three keep it.

Not restated: the pixel-parallel schedule's padded balls around spheres and blocks of spheres
(pixel.hip).  They are reachable only through a render; tests/test_gpu_adversarial.py renders the
sphere scene through them from the edge of the domain on the device.

float32 throughout, one rounding per operation, an fma where the device uses one (`fma32`);
vectorised over the rays.
"""
import numpy as np

from xraytracer_amd import abi

F = np.float32
INF = F(np.inf)
FLT_MAX = np.finfo(F).max
K_OBJ, K_BVH = F(1e-3), F(1e-4)    # Bounds::pad's factor: object boxes; triangle and sphere BVHs
SMALL_TRIS, SMALL_OBJS, LARGE_OBJ_TRIS, SPH_BVH_MIN = 1024, 256, 256, 16   # wavefront.h


# ------------------------------------------------------------------ the host's boxes ----
def pad(lo, hi, k):
    """Bounds::pad: k * diag + k, every operation in float"""
    d = (np.asarray(hi, F) - np.asarray(lo, F)).astype(F)
    diag = np.sqrt(F(F(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]))
    return F(F(F(k) * F(diag)) + F(k))


def plane_tri_ok(e1, e2, a):
    if e1[a] != 0.0 or e2[a] != 0.0:
        return False
    p, q = (a + 1) % 3, (a + 2) % 3
    for x in (e1[p], e1[q], e2[p], e2[q]):
        if x != 0.0 and not (abs(x) >= F(1e-6) and abs(x) <= F(1e5)):
            return False
    A, B = float(e1[p]) * float(e2[q]), float(e1[q]) * float(e2[p])
    return abs(A - B) > 1e-4 * (abs(A) + abs(B))


class Culls:
    """What upload_scene_one builds for culling out of a SceneBundle's description.

    kind                         "tri", "sphere" or "mixed" (upload_flat's scene_kind)
    small, two_level, bvh, sphere_bvh   which structures the scene gets
    obj_first[k], obj_count[k]   object k's triangles in the device's packed order
    obj_lo, obj_hi [n_objs, 3]   padded object boxes (NaN rows: the object has none)
    plane_axis[k], plane_c[k]    DObjPlane (axis -1: none)
    tri_lo, tri_hi [T, 3]        padded per-triangle boxes of the BVH's triangles (NaN: not in it)
    tri_in_bvh [T]               the triangle is walked through the BVH
    tri_dropped [T]              ... or left out of it for a zero edge vector
    sph_lo, sph_hi [S, 3]        padded per-sphere boxes (sphere BVH); s_lo, s_hi: unpadded
    pad_obj, pad_bvh             the margins used
    force_bvh: build the one-level BVH's boxes although the scene is small (what the same triangles
    would get inside a larger scene's BVH with these bounds)."""

    def __init__(self, scene, force_bvh=False):
        d = scene.desc
        objs = [d.objects[k] for k in range(d.n_objects)]
        tv = scene.triangles()
        self.n_objs = len(objs)
        self.obj_first, self.obj_count, order = [], [], []
        kinds = set()
        for o in objs:
            self.obj_first.append(len(order))
            if o.kind == abi.XRT_OBJ_MESH:
                order += list(range(o.first, o.first + o.count))
                self.obj_count.append(int(o.count))
            else:
                self.obj_count.append(0)
            if o.count > 0:
                kinds.add(int(o.kind))
        self.obj_first = np.asarray(self.obj_first, int)
        self.mesh_count = np.asarray(self.obj_count, int)
        tv = tv[order] if len(order) else np.zeros((0, 3, 3), F)
        self.v0 = tv[:, 0].astype(F)
        self.e1 = (tv[:, 1] - tv[:, 0]).astype(F)          # Src/primitive.cpp:142-143, on the host
        self.e2 = (tv[:, 2] - tv[:, 0]).astype(F)
        vs = np.stack([self.v0, (self.v0 + self.e1).astype(F), (self.v0 + self.e2).astype(F)])   # tri_box
        self.t_lo, self.t_hi = vs.min(0), vs.max(0)
        T = len(tv)
        self.kind = "tri" if kinds <= {abi.XRT_OBJ_MESH} else ("sphere" if kinds == {abi.XRT_OBJ_SPHERE} else "mixed")
        nan3 = lambda n: np.full((n, 3), np.nan, F)
        self.obj_lo, self.obj_hi = nan3(self.n_objs), nan3(self.n_objs)
        self.tri_lo, self.tri_hi = nan3(T), nan3(T)
        self.tri_in_bvh, self.tri_dropped = np.zeros(T, bool), np.zeros(T, bool)
        self.pad_obj = self.pad_bvh = None
        # DObjPlane per mesh object (flatten_scene)
        self.plane_axis, self.plane_c = np.full(self.n_objs, -1), np.zeros(self.n_objs, F)
        for k, o in enumerate(objs):
            if o.kind != abi.XRT_OBJ_MESH or o.count == 0:
                continue
            f, c = self.obj_first[k], o.count
            for a in range(3):
                first = tv[f, 0, a]
                if np.all(tv[f:f + c, :, a] == first) and all(plane_tri_ok(self.e1[t], self.e2[t], a) for t in range(f, f + c)):
                    self.plane_axis[k], self.plane_c[k] = a, first
                    break
        self.small = self.kind == "tri" and 0 < T <= SMALL_TRIS and self.n_objs <= SMALL_OBJS
        self.two_level = self.bvh = self.sphere_bvh = False
        self.forced = bool(force_bvh and self.small)
        if self.small:
            self._object_boxes(range(self.n_objs), np.arange(T))
        if self.kind == "tri" and T > 0 and (not self.small or force_bvh):
            self._tri_bvh(allow_two_level=not self.small)
        # sphere BVH
        ns = int(d.n_spheres)
        self.sph_lo, self.sph_hi = nan3(ns), nan3(ns)
        if self.kind == "sphere" and ns >= SPH_BVH_MIN:
            # flatten_scene packs the spheres object by object; one sphere per object, in order
            sp = np.ctypeslib.as_array(d.spheres, shape=(ns * 4,)).reshape(-1, 4)
            idx = [o.first + i for o in objs if o.kind == abi.XRT_OBJ_SPHERE for i in range(o.count)]
            sp = sp[idx].astype(F)
            r = np.abs(sp[:, 3:4])
            lo, hi = (sp[:, :3] - r).astype(F), (sp[:, :3] + r).astype(F)
            self.pad_bvh = pad(lo.min(0), hi.max(0), K_BVH)
            self.s_lo, self.s_hi = lo, hi          # as build_sphere_bvh hands them to the build
            self.sph_lo, self.sph_hi = (lo - self.pad_bvh).astype(F), (hi + self.pad_bvh).astype(F)
            self.sph_first = np.cumsum([0] + [o.count if o.kind == abi.XRT_OBJ_SPHERE else 0 for o in objs])[:-1]
            self.sphere_bvh = True

    def _object_boxes(self, objects, bound_tris):
        """object_box + pad_boxes: boxes of `objects`, margin from the bounds of `bound_tris`"""
        self.pad_obj = pad(self.t_lo[bound_tris].min(0), self.t_hi[bound_tris].max(0), K_OBJ)
        for k in objects:
            f, c = self.obj_first[k], self.mesh_count[k]
            lo = self.t_lo[f:f + c].min(0) if c else np.full(3, 3e38, F)
            hi = self.t_hi[f:f + c].max(0) if c else np.full(3, -3e38, F)
            self.obj_lo[k], self.obj_hi[k] = (lo - self.pad_obj).astype(F), (hi + self.pad_obj).astype(F)

    def _tri_bvh(self, allow_two_level):
        T = len(self.v0)
        big, small_objs = [], []
        for k in range(self.n_objs):
            f, c = self.obj_first[k], self.mesh_count[k]
            if c > LARGE_OBJ_TRIS:
                big += list(range(f, f + c))
            elif c > 0:
                small_objs.append(k)
        n_small = int(sum(self.mesh_count[k] for k in small_objs))
        two = allow_two_level and bool(big) and bool(small_objs) and n_small <= SMALL_TRIS and len(small_objs) <= SMALL_OBJS
        if not two:
            big = list(range(T))
        big = np.asarray(big, int)
        zero = np.all(self.e1[big] == 0.0, axis=1) | np.all(self.e2[big] == 0.0, axis=1)
        if not np.all(zero):
            self.tri_dropped[big[zero]] = True
            big = big[~zero]
        bound = big
        if two:
            bound = np.concatenate([big] + [np.arange(self.obj_first[k], self.obj_first[k] + self.mesh_count[k]) for k in small_objs])
            self._object_boxes(small_objs, bound)
        self.pad_bvh = pad(self.t_lo[bound].min(0), self.t_hi[bound].max(0), K_BVH)
        self.tri_lo[big] = (self.t_lo[big] - self.pad_bvh).astype(F)
        self.tri_hi[big] = (self.t_hi[big] + self.pad_bvh).astype(F)
        self.tri_in_bvh[big] = True
        self.two_level, self.bvh = two, True


# ------------------------------------------------------------------ the device's tests ----
def rcp_variants(d):
    """1 / d as the correctly rounded float and its two float neighbours (v_rcp_f32 is accurate
    to 1 ulp); an infinite reciprocal (d = +-0) stays what it is in all three"""
    d = np.asarray(d, F)
    with np.errstate(divide="ignore", over="ignore"):
        r = (F(1.0) / d).astype(F)
    keep = np.isinf(r)
    return [r, np.where(keep, r, np.nextafter(r, -INF)).astype(F), np.where(keep, r, np.nextafter(r, INF)).astype(F)]


def fma32(a, b, c):
    """fma(a, b, c) with one float32 rounding.  The product of two floats is exact in double; the sum
    is taken in double with its rounding error (two-sum) and rounded to odd, which makes the final
    rounding to float32 the correct single one.  |a * b| and |c| stay far below double's range here."""
    p = np.asarray(a, np.float64) * np.asarray(b, np.float64)
    c = np.asarray(c, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        odd = (s.view(np.int64) & 1) == 1
        fix = np.isfinite(s) & (err != 0.0) & ~odd
        s = np.where(fix, np.nextafter(s, np.where(err > 0.0, np.inf, -np.inf)), s)
        return s.astype(F)


def _near_far(t0, t1, tlim):
    tn = np.fmax(np.fmax(np.fmin(t0[:, 0], t1[:, 0]), np.fmin(t0[:, 1], t1[:, 1])), np.fmax(np.fmin(t0[:, 2], t1[:, 2]), F(0.0)))
    tf = np.fmin(np.fmin(np.fmax(t0[:, 0], t1[:, 0]), np.fmax(t0[:, 1], t1[:, 1])), np.fmin(np.fmax(t0[:, 2], t1[:, 2]), tlim))
    return tn, tf


def _slabs(o, inv, lo, hi):
    with np.errstate(invalid="ignore", over="ignore"):
        return ((lo - o).astype(F) * inv).astype(F), ((hi - o).astype(F) * inv).astype(F)


def box_overlap(o, inv, lo, hi, tlim):
    """path_common.h box_overlap = lscene.h bvh_box: does [0, tlim] overlap the box?"""
    tn, tf = _near_far(*_slabs(o, inv, lo, hi), tlim)
    return ~(tn > tf)


def bvh_enter(o, inv, lo, hi, tlim):
    """path_common.h bvh_enter: the entry distance, inf when it misses (the walk enters on != inf)"""
    tn, tf = _near_far(*_slabs(o, inv, lo, hi), tlim)
    return np.where(tn > tf, INF, tn).astype(F)


def obj_overlap(o, inv, lo, hi, tlim):
    """merged.h obj_overlap = box_overlap_f; inv: the unclamped reciprocal (rcpc clamps it here)"""
    inv = np.clip(inv, F(-1e30), F(1e30)).astype(F)        # v_med3_f32(rcp, -1e30, 1e30)
    with np.errstate(over="ignore"):
        oi = (o * inv).astype(F)
    tn, tf = _near_far(fma32(lo, inv, -oi), fma32(hi, inv, -oi), tlim)
    return ~(tn > tf)


def plane_away(o, d, axis, c):
    """merged.h plane_away = bvh_walk.h plane_away_w, per ray with its object's (axis, c)"""
    n = np.arange(len(o))
    a = np.maximum(axis, 0)
    with np.errstate(invalid="ignore"):
        return (axis >= 0) & ((((o[n, a] - c).astype(F)) * d[n, a]).astype(F) >= F(0.0))


# ------------------------------------------------------------------ the check ----
def culled_hits(culls, rays, obj, prim, t):
    """For the rays the oracle hits (obj[n] >= 0: object, prim[n]: the triangle within it or -1,
    t[n]): which of them would one of the scene's culls have dropped?  Returns {test name: bool [n]}
    over all rays (False where the oracle misses or the test does not apply to the hit object).
    Tests on padded object boxes are named "obj:...", on the 1e-4 boxes "bvh:...", the plane cull
    "plane"."""
    rays = np.asarray(rays, F)
    o, d = rays[:, :3], rays[:, 3:]
    obj, prim, t = np.asarray(obj), np.asarray(prim), np.asarray(t, F)
    n = len(rays)
    hit = obj >= 0
    j = np.where(hit, obj, 0)
    out = {}
    invs = rcp_variants(d)
    tmax = np.full(n, FLT_MAX, F)

    def all_keep(fn, lo, hi, tlim):
        keep = np.ones(n, bool)
        for inv in invs:
            keep &= fn(o, inv, lo, hi, tlim)
        return keep

    has_box = hit & ~np.isnan(culls.obj_lo[j, 0])
    if has_box.any():
        lo, hi = culls.obj_lo[j], culls.obj_hi[j]
        for name, fn in (("box_overlap", box_overlap), ("obj_overlap", obj_overlap)):
            out[f"obj:{name}@t"] = has_box & ~all_keep(fn, lo, hi, t)
            out[f"obj:{name}@max"] = has_box & ~all_keep(fn, lo, hi, tmax)
        out["plane"] = has_box & plane_away(o, d, culls.plane_axis[j], culls.plane_c[j])
    if culls.bvh:
        tri = np.where(hit & (prim >= 0), culls.obj_first[j] + np.maximum(prim, 0), 0)
        walked = hit & (prim >= 0) & (culls.forced | np.isnan(culls.obj_lo[j, 0]))
        inb = walked & culls.tri_in_bvh[tri]
        enter = lambda o_, inv, lo, hi, tl: bvh_enter(o_, inv, lo, hi, tl) != INF
        with np.errstate(invalid="ignore"):
            out["bvh:bvh_enter@t"] = inb & ~all_keep(enter, culls.tri_lo[tri], culls.tri_hi[tri], t)
        out["bvh:left_out"] = walked & ~culls.tri_in_bvh[tri]     # a hit on a triangle the BVH does not hold
    if culls.sphere_bvh:
        s = np.where(hit, culls.sph_first[j], 0)
        with np.errstate(invalid="ignore"):
            out["bvh:bvh_box@t"] = hit & ~all_keep(box_overlap, culls.sph_lo[s], culls.sph_hi[s], t)
    return out


def count_by_structure(culled):
    """hits dropped per structure: "obj" (a test on the 1e-3 object boxes, or the plane cull),
    "tri_bvh" and "sphere_bvh" (the 1e-4 boxes)"""
    n = {"obj": 0, "tri_bvh": 0, "sphere_bvh": 0}
    for name, m in culled.items():
        key = "sphere_bvh" if name == "bvh:bvh_box@t" else ("tri_bvh" if name.startswith("bvh:") else "obj")
        n[key] += int(np.count_nonzero(m))
    return n


# ------------------------------------------------------------------ the measured domain ----
# The smallest k at which a hit of the oracle's is dropped when ray origins ("far") or the scene
# itself ("shifted") lie 2^k scene diagonals from the scene's centre resp. the world origin, per
# structure, over tests/adversarial_rays.py's scenes and k = 0, 2, ..., 16.  Measured by
# tests/test_adversarial_rays.py::test_k_fail (python -m pytest tests/test_adversarial_rays.py -s -k k_fail
# prints the counts), which fails when a change moves one of them.  The shifted scene is small, so
# the device gives it object boxes only; its "tri_bvh" row is what the same triangles would get in a
# larger scene's BVH with the same bounds.  There is no shifted sphere scene.
K_FAIL = {
    ("obj", "far"): 12, ("obj", "shifted"): 16,
    ("tri_bvh", "far"): 6, ("tri_bvh", "shifted"): 12,
    ("sphere_bvh", "far"): 2,
}
# Two octaves below the first failure, because a sampled family does not find the worst ray.
# EXACT_DIAGONALS holds for every scene; the sphere BVH sets it (Sphere::intersect's own float error
# grows with the distance and passes the margin first).  Scenes of triangles only reach further.
EXACT_DIAGONALS = 2.0 ** (min(K_FAIL.values()) - 2)
EXACT_DIAGONALS_TRI = 2.0 ** (min(v for (s, _), v in K_FAIL.items() if s != "sphere_bvh") - 2)


def exact_diagonals(kind):
    """the domain of a scene of Culls.kind `kind`, in scene diagonals"""
    return EXACT_DIAGONALS_TRI if kind == "tri" else EXACT_DIAGONALS
