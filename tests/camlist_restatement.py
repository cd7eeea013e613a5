"""The camera lists (k_camlist, xraytracer_amd/csrc/spec.hip) restated in numpy float32 — a test
helper, not a test file, in the style of tests/whitted_restatement.py.  It shares no code with
the device.

Every camera ray of a pixel (Src/renderer.cpp:44-50: u = (j + r) / W, v = (i + r') / H with
r, r' in [0, 1)) leaves the eye o inside the cone over the corner directions of the pixel's
jitter square, widened by 0.01 pixel.  The list of a pixel makes three claims:

  membership (`possible_hits`, `mask`)  A triangle is left out when the cone and the triangle's
      cone from o are separated by one of the cone's four side planes or one of the triangle's
      three edge planes through o, each by a margin of 1e-4 of the vectors' scale.  A pixel is
      *empty* when no triangle survives (`empty_pixels`): the merged schedule finishes it
      without tracing it, as spp samples of one segment, two draws and radiance +0 each.
  the beyond-cover cull (`cover`, `keep`)  A triangle that every corner ray of the cone hits
      (Moller-Trumbore, barycentric margin 1e-3, |det| above 1e-6 |e1| |e2| |D|) covers the
      pixel; a listed triangle whose three vertices lie beyond a covering triangle's plane, as
      seen from o, by more than 1e-4 |n| (|q - p0| + |o - p0|) is dropped from the list.
  the covering shortcut (`covering`)  When one triangle is left and it covers the pixel, the
      device takes it as the first hit of every camera ray of the pixel with no test at all.

`camera_lists` gives all of it per slot, with the four words the device stores.
tests/test_camlist_restatement.py checks the claims against the oracle on a machine with no
GPU; tests/test_gpu_camlist.py compares the device's lists (xrt_test_camlist) with these word for
word, and tests/test_gpu_elide.py checks the device's retirement of the empty pixels.

float32 throughout, one rounding per operation, sums in the device's order (dot: x*x' + y*y'
+ z*z', left to right); vectorised over the pixels, one triangle at a time.
"""
import collections

import numpy as np

F = np.float32
MARGIN = F(0.01)   # pixels: the jitter square's widening
TOL = F(1e-4)      # the separating planes' margin, and the beyond-cover cull's
BARY = F(1e-3)     # the barycentric margin of "covers"
DET = F(1e-6)      # ... and its determinant floor, of |e1| |e2| |D|


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], axis=-1).astype(F)


def _length(a):
    return np.sqrt(_dot(a, a)).astype(F)


def corner_dirs(camera, width, height, rows, cols):
    """the widened jitter square's corner directions D0..D3 [n, 4, 3] of the pixels (rows[n],
    cols[n]): PinholeCamera::sampleRay's direction (Src/camera.h:49-58), not normalised"""
    c2w = np.asarray(camera.c2w, F)
    scale, aspect = F(camera.scale), F(camera.aspect)
    fw, fh = F(width), F(height)
    col, row = np.asarray(cols, F), np.asarray(rows, F)
    u0 = (col - MARGIN) / fw
    u1 = (col + (F(1.0) + MARGIN)) / fw
    v0 = (row - MARGIN) / fh
    v1 = (row + (F(1.0) + MARGIN)) / fh

    def world(u, v):
        dx = (F(2.0) * u - F(1.0)) * scale
        dy = (F(1.0) - F(2.0) * v) * scale / aspect
        dz = np.full_like(dx, F(-1.0))
        return np.stack([(dx * c2w[0] + dy * c2w[4]) + dz * c2w[8],
                         (dx * c2w[1] + dy * c2w[5]) + dz * c2w[9],
                         (dx * c2w[2] + dy * c2w[6]) + dz * c2w[10]], axis=-1).astype(F)

    return np.stack([world(u0, v0), world(u1, v0), world(u1, v1), world(u0, v1)], axis=1)


def possible_hits(camera, tri_v, width, height, rows, cols):
    """[n, T] bool: may a camera ray of pixel n hit triangle t?  tri_v: [T, 3, 3] float32
    vertices (SceneBundle.triangles())."""
    tri_v = np.asarray(tri_v, F).reshape(-1, 3, 3)
    D = corner_dirs(camera, width, height, rows, cols)
    n_pix = D.shape[0]
    o = np.asarray(camera.c2w, F)[12:15]
    Dc = (D[:, 0] + D[:, 1]) + (D[:, 2] + D[:, 3])
    side_n = np.zeros((n_pix, 4, 3), F)   # the cone's side planes: unit normals pointing inwards
    Dl = np.zeros((n_pix, 4), F)
    for k in range(4):
        nk = _cross(D[:, k], D[:, (k + 1) & 3])
        sg = np.where(_dot(nk, Dc) < F(0.0), F(-1.0), F(1.0)).astype(F)
        fac = sg / _length(nk)
        side_n[:, k] = nk * fac[:, None]
        Dl[:, k] = _length(D[:, k])
    keep = np.zeros((n_pix, len(tri_v)), bool)
    for t, (v0, v1, v2) in enumerate(tri_v):
        e1 = v1 - v0   # the device's triangle record: p0, e1, e2 (Src/primitive.cpp:142-143)
        e2 = v2 - v0
        a = np.stack([v0 - o, (v0 + e1) - o, (v0 + e2) - o]).astype(F)
        al = _length(a)
        out = np.zeros(n_pix, bool)
        for k in range(4):
            every = np.ones(n_pix, bool)
            for q in range(3):
                every &= _dot(side_n[:, k], a[q][None, :]) < -TOL * (al[q] + F(1.0))
            out |= every
        for e in range(3):
            pa, pb, pc = a[e], a[(e + 1) % 3], a[(e + 2) % 3]
            pn = _cross(pa, pb)
            sc = al[e] * al[(e + 1) % 3]
            side = _dot(pn, pc)
            if not abs(side) > TOL * sc * al[(e + 2) % 3]:
                continue   # the eye lies near the triangle's plane: no edge plane decides
            if side < F(0.0):
                pn = pn * F(-1.0)
            every = np.ones(n_pix, bool)
            for k in range(4):
                every &= _dot(pn[None, :], D[:, k]) < -TOL * sc * Dl[:, k]
            out |= every
        keep[:, t] = ~out
    return keep


def empty_pixels(scene, width, height, shard_index=0, shard_count=1):
    """[height, width] bool: the pixels the merged schedule finishes untraced (rows the shard
    does not own: False)"""
    rows = np.arange(shard_index, height, shard_count)
    rr, cc = np.meshgrid(rows, np.arange(width), indexing="ij")
    tris = scene.triangles()
    out = np.zeros((height, width), bool)
    if len(tris) == 0:
        out[rows] = True
        return out
    keep = possible_hits(scene.camera, tris, width, height, rr.ravel(), cc.ravel())
    out[rr.ravel(), cc.ravel()] = ~keep.any(axis=1)
    return out


def device_triangles(scene):
    """[T, 3, 3] float32: the scene's triangles in the device's order — object by object in the
    description's object order (flatten_scene), which is the order Scene::intersect scans them in
    and the index the lists' bits and `covering` name"""
    tris, d = scene.triangles(), scene.desc
    parts = [tris[d.objects[k].first:d.objects[k].first + d.objects[k].count] for k in range(d.n_objects)
             if d.objects[k].kind == 0]   # XRT_OBJ_MESH (area lights are meshes too)
    return np.concatenate(parts) if parts else np.zeros((0, 3, 3), F)


def covers(camera, tri_v, width, height, rows, cols):
    """[n, T] bool: does every corner ray of pixel n's cone hit triangle t well inside?"""
    tri_v = np.asarray(tri_v, F).reshape(-1, 3, 3)
    D = corner_dirs(camera, width, height, rows, cols)
    o = np.asarray(camera.c2w, F)[12:15]
    Dl = np.stack([_length(D[:, k]) for k in range(4)], axis=1)
    cov = np.ones((D.shape[0], len(tri_v)), bool)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):   # det 0: inf / NaN fail the comparisons
        for t, (p0, v1, v2) in enumerate(tri_v):
            e1 = v1 - p0
            e2 = v2 - p0
            tvec = o - p0
            qvec = _cross(tvec, e1)
            floor = (DET * _length(e1)) * _length(e2)
            for k in range(4):
                pvec = _cross(D[:, k], e2[None, :])
                det = _dot(e1[None, :], pvec)
                uu = _dot(tvec[None, :], pvec) / det
                vv = _dot(D[:, k], qvec[None, :]) / det
                tt = _dot(e2, qvec) / det
                cov[:, t] &= ((np.abs(det) > floor * Dl[:, k]) & (uu >= BARY) & (vv >= BARY) &
                              (uu + vv <= F(1.0) - BARY) & (tt > F(0.0)))
    return cov


def beyond_planes(camera, tri_v):
    """[T, T] bool: entry (t, t2) — does triangle t2 lie wholly beyond triangle t's plane, as seen
    from the eye, by the cull's margin?  (The vertices as the device forms them: p0, p0 + e1,
    p0 + e2.)  It depends on no pixel; the diagonal is False."""
    tri_v = np.asarray(tri_v, F).reshape(-1, 3, 3)
    o = np.asarray(camera.c2w, F)[12:15]
    n_tri = len(tri_v)
    e1 = tri_v[:, 1] - tri_v[:, 0]
    e2 = tri_v[:, 2] - tri_v[:, 0]
    qs = np.stack([tri_v[:, 0], tri_v[:, 0] + e1, tri_v[:, 0] + e2], axis=1)   # [T, 3, 3]
    out = np.zeros((n_tri, n_tri), bool)
    for t in range(n_tri):
        p0 = tri_v[t, 0]
        nt = _cross(e1[t], e2[t])
        ntl = _length(nt)
        so = _dot(nt, o - p0)
        sg = F(-1.0) if so < F(0.0) else F(1.0)
        ol = _length(o - p0)
        far = np.full(n_tri, bool(so != F(0.0)))
        for q in range(3):
            w = qs[:, q] - p0[None, :]
            far &= sg * _dot(nt[None, :], w) < (-TOL * ntl) * (_length(w) + ol)
        far[t] = False
        out[t] = far
    return out


CameraLists = collections.namedtuple("CameraLists", "mask cover keep covering words")


def camera_lists(scene, width, height, shard_index=0, shard_count=1):
    """The camera lists of the shard's slots, in slot order (slot s: column s % width, row
    shard_index + shard_count * (s // width)), T the scene's triangles (device_triangles, at
    most 64):
      mask     [n, T] bool   membership: the triangles a camera ray of the pixel may hit
      cover    [n, T] bool   of those, the ones that cover the pixel
      keep     [n, T] bool   the list: mask less what lies beyond a covering triangle's plane
      covering [n] int32     the list's only triangle where it covers the pixel, else -1
      words    [n, 4] uint32 what the device stores: keep's bits 0-31, 32-63, covering, 0"""
    tris = device_triangles(scene)
    n_tri = len(tris)
    assert n_tri <= 64, n_tri
    rows = np.arange(shard_index, height, shard_count)
    rr, cc = np.meshgrid(rows, np.arange(width), indexing="ij")
    rr, cc = rr.ravel(), cc.ravel()
    mask = possible_hits(scene.camera, tris, width, height, rr, cc)
    cover = covers(scene.camera, tris, width, height, rr, cc) & mask
    beyond = beyond_planes(scene.camera, tris)
    hidden = (cover[:, :, None] & beyond[None, :, :]).any(axis=1)   # [n, t2]: beyond some covering t
    keep = mask & ~hidden
    only = keep.sum(axis=1) == 1
    first = np.argmax(keep, axis=1)
    covering = np.where(only & (keep & cover).any(axis=1), first, -1).astype(np.int32)
    bits = (keep.astype(np.uint64) << np.arange(n_tri, dtype=np.uint64)[None, :]).sum(axis=1, dtype=np.uint64)
    words = np.zeros((len(rr), 4), np.uint32)
    words[:, 0] = (bits & np.uint64(0xffffffff)).astype(np.uint32)
    words[:, 1] = (bits >> np.uint64(32)).astype(np.uint32)
    words[:, 2] = covering.view(np.uint32)
    return CameraLists(mask, cover, keep, covering, words)


def classes(lists):
    """the pixels of each kind, [n] bool each: empty (nothing listed), covered (the shortcut: no
    test), multi (two or more listed), single (one listed, not covering: tested), culled (the
    beyond-cover cull dropped something), tied (two or more listed triangles cover the pixel)"""
    n_keep = lists.keep.sum(axis=1)
    return dict(empty=n_keep == 0, covered=lists.covering >= 0, multi=n_keep >= 2,
                single=(n_keep == 1) & (lists.covering < 0), culled=(lists.mask & ~lists.keep).any(axis=1),
                tied=(lists.keep & lists.cover).sum(axis=1) >= 2)
