"""The emptiness test of the camera lists (k_camlist, xraytracer_amd/csrc/spec.hip) restated in
numpy float32 — a test helper, not a test file, in the style of tests/whitted_restatement.py.
It shares no code with the device.

A pixel is *empty* when no triangle of the scene survives the list's separating-plane tests:
every camera ray of the pixel (Src/renderer.cpp:44-50: u = (j + r) / W, v = (i + r') / H with
r, r' in [0, 1)) leaves the eye o inside the cone over the corner directions of the pixel's
jitter square, widened by 0.01 pixel.  A triangle is left out when the cone and the triangle's
cone from o are separated by one of the cone's four side planes or one of the triangle's three
edge planes through o, each by a margin of 1e-4 of the vectors' scale.  The merged schedule
finishes an empty pixel without tracing it: spp samples of one segment, two draws and radiance
+0 each.  tests/test_camlist_restatement.py checks that claim against the oracle on a machine
with no GPU; tests/test_gpu_elide.py checks the device's result.

float32 throughout, one rounding per operation, sums in the device's order (dot: x*x' + y*y'
+ z*z', left to right); vectorised over the pixels, one triangle at a time.
"""
import numpy as np

F = np.float32
MARGIN = F(0.01)   # pixels: the jitter square's widening
TOL = F(1e-4)      # the separating planes' margin


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
