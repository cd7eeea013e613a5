"""Irregular meshes for the hierarchy builds and the kernels that walk them — a helper, not a test
file, in the style of tests/matless_scenes.py.  Every other BVH of the suite comes from a tessellated
sphere, the Cornell box or a grid of spheres: even, shallow trees.  These are built to be uneven, in
deterministic numpy, and each is held against a walk's limit (csrc/wavefront.h: kBvhStack = 24 entries
of the binary walk, kBvh4Stack = 48 of the 4-wide one, kBvhTopNodes = 64 nodes kept in LDS,
kBvhLeafTri = 4 triangles per leaf):

  spiral(octaves, diagonal)
                      N_SPIRAL triangles at x_k = TOP * 2^(-k * octaves / N_SPIRAL) along the x axis, or
                      along the diagonal x = y = z, each of size 0.3 x_k: SAH peels a bin off per level,
                      so the first build is as deep as the walks allow or deeper (SPIRALS below).  The
                      top twenty octaves can be hit (|det| >= FLT_EPSILON needs an edge of about
                      2^-11); the padded boxes near the origin all overlap.
  concentric          triangles whose boxes share one centre exactly: the centroid extent is 0 and the
                      build splits at the median from the root down
  clumps              nine tenths of the triangles in a cluster a thousandth of the scene wide, the
                      rest scattered; slivers of aspect 1e4; collinear triangles (non-zero edges: in
                      the BVH; det is an exact 0, so never hit); triangles with an exactly zero edge (left out of the BVH)
  counts_63/64/65     strips whose trees have exactly that many nodes, around kBvhTopNodes; `one_leaf`:
                      three triangles in all, a root with one leaf and an empty right child.  The rest
                      of each mesh are zero-edge triangles, which make the scene large enough for a BVH.
  allcounts_63/64/65  the same for the one-level form: the tree over the strip and the box together
  spheres_irregular   spheres with geometric radii and positions, nested and concentric ones among
                      them (the threaded sphere BVH, kSphBvhMin = 16)

A triangle family comes in two forms beside the Cornell box and its light: "two" — the mesh as one
object of more than kLargeObjTris triangles, which makes the scene two-level (the mesh in the BVH,
the box's objects scanned) — and "one" — the mesh cut into objects of at most 250 triangles, more
than kSmallTris in all, so there is no large object and every triangle of the scene is in one BVH
(tests/whitted_bvh_scenes.py medium_meshes' pattern).

boxes(scene) gives what build_tri_bvh hands to the build, restated by cull_restatement.Culls;
write_boxes writes it in the format tests/cpp/bvh_kat.cpp reads.  rays(name) is the ray set of the
query tests: a third from the deep end of the mesh outward, a third aimed at triangles that can be
hit, a third random with axis-parallel components."""
import functools
import os
import re
import struct
import subprocess

import numpy as np

import pyoracle
import whitted_scenes as ws
from cull_restatement import Culls
from matless_scenes import QUAD_LIGHT
from xraytracer_amd import scenes

F = np.float32
N_SPIRAL = 1100
TOP = 256.0          # the largest triangle's position: inside the Cornell box
MESH = "irregular"
LEAF_TRI = 4         # tuning.h XRT_BVH_LEAF
# the Cornell camera's orientation from just outside the origin corner of the box, the deep end of the
# spirals: the padded boxes there overlap within about 0.1, which is a third of this image's width
DEEP_C2W = (-1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, -1.0, 0, 0.04, 0.05, -0.25, 1)
# ... and from the open front of the box at the height of the strips, which span the image's width
STRIP_C2W = (-1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, -1.0, 0, 280.0, 440.0, -140.0, 1)


# ------------------------------------------------------------------ triangles ----
def corner_triangles(p, s):
    """one triangle per row of p [n, 3] and s [n]: vertices p + s e_x, p + s e_y, p + s e_z, whose box
    is [p, p + s] in every axis, in float"""
    p = np.asarray(p, F)
    s = np.asarray(s, F)[:, None]
    v = np.repeat(p[:, None, :], 3, axis=1)
    for q in range(3):
        v[:, q, q] = (p[:, q:q + 1] + s)[:, 0].astype(F)
    return v.astype(F)


def spiral_triangles(octaves, diagonal):
    k = np.arange(N_SPIRAL, dtype=np.float64)
    x = (TOP * 2.0 ** (-k * octaves / N_SPIRAL)).astype(F)
    p = np.stack([x, x if diagonal else np.zeros_like(x), x if diagonal else np.zeros_like(x)], axis=1)
    return corner_triangles(p, (F(0.3) * x).astype(F))


def concentric_triangles(n=1200):
    """triangle k spans [c - r_k, c + r_k] in every axis with c and r_k powers of two and sums that are
    exact in float, so every box centre 0.5 * (min + max) is c bit for bit; three orientations"""
    c = np.array([128.0, 128.0, 256.0], F)
    r = (64.0 * 2.0 ** (-(np.arange(n) % 400) / 50.0)).astype(F)      # 8 octaves, three triangles per radius
    r = (np.round(r * 1024.0) / 1024.0).astype(F)                      # multiples of 2^-10: c +- r is exact
    v = np.zeros((n, 3, 3), F)
    for k in range(n):
        a = k // 400
        lo, hi = c - r[k], c + r[k]
        # two opposite corners and a third vertex at a face centre: the box is [lo, hi]
        v[k, 0], v[k, 1] = lo, hi
        third = c.copy()
        third[a] = lo[a]
        third[(a + 1) % 3] = hi[(a + 1) % 3]
        v[k, 2] = third
    return v


def clump_triangles(n=2000, seed=17):
    rng = np.random.default_rng(seed)
    n_far = n // 10
    n_in = n - n_far
    # the cluster: 0.4 wide at (200, 120, 300); the rest over 400 in every axis
    p = np.concatenate([rng.uniform(0.0, 0.4, (n_in, 3)) + (200.0, 120.0, 300.0), rng.uniform(40.0, 440.0, (n_far, 3))])
    s = np.concatenate([rng.uniform(0.01, 0.05, n_in), rng.uniform(5.0, 40.0, n_far)])
    v = np.repeat(p[:, None, :], 3, axis=1)
    v[:, 1] += rng.normal(size=(n, 3)) * s[:, None]
    v[:, 2] += rng.normal(size=(n, 3)) * s[:, None]
    kind = np.zeros(n, int)
    sl = np.arange(0, n, 7)              # slivers: the second edge 1e-4 of the first, across it
    e1 = v[sl, 1] - v[sl, 0]
    across = np.cross(e1, (0.0, 1.0, 0.3))
    v[sl, 2] = v[sl, 0] + 0.5 * e1 + 1e-4 * across
    kind[sl] = 1
    v = v.astype(F)
    co = np.arange(3, n, 31)             # collinear along an axis: e1 and e2 have one non-zero component, the
    for i in co:                         # same one, so det = e1 . (d x e2) is an exact 0 for every direction
        a = int(i) % 3
        v[i, 1], v[i, 2] = v[i, 0], v[i, 0]
        v[i, 1, a] += F(s[i])
        v[i, 2, a] += F(2.0 * s[i])
    kind[co] = 2
    ze = np.arange(5, n, 97)             # an exactly zero edge: two equal vertices
    v[ze, 1 + (ze % 2)] = v[ze, 0]
    kind[ze] = 3
    return v, kind


STRIP_HEIGHT = 120.0


def strip_triangles(n):
    """n equal triangles in a row along x across the box, above its blocks, 0.75 of their spacing wide
    and deep and STRIP_HEIGHT tall: a ribbon side-on to STRIP_C2W, five pixel rows high at W x H, so
    camera rays fall on every part of it"""
    k = np.arange(n, dtype=np.float64)
    p = np.stack([40.0 + k * (480.0 / n), np.full(n, 400.0), np.full(n, 300.0)], axis=1).astype(F)
    v = corner_triangles(p, np.full(n, 480.0 / n * 0.75, F))
    v[:, 1, 1] = F(400.0 + STRIP_HEIGHT)
    return v


def with_zero_edge(v, total):
    """v and total - len(v) triangles with an exactly zero edge, which build_tri_bvh leaves out"""
    z = np.repeat(v[:1], total - len(v), axis=0).copy()
    z[:, 1] = z[:, 0]
    return np.concatenate([v, z]).astype(F)


# strips whose BVH (leaves of at most 4) has exactly this many nodes: in the two-level form over the
# strip alone (counts_N), in the one-level form over the strip and the box's 36 triangles (allcounts_N);
# tests/test_bvh_build.py holds the host program's node counts to the names
STRIP_FOR_NODES = {63: 256, 64: 257, 65: 258}
STRIP_FOR_ALL_NODES = {63: 154, 64: 155, 65: 156}


# ------------------------------------------------------------------ scenes ----
def cornell_with(tri_v, form, w, h, material="lambert", camera=DEEP_C2W):
    """the Cornell box, its light and the mesh: form "two" as one object, "one" in objects of 250"""
    s = scenes.SceneBundle()
    s.load_obj(scenes.CORNELL_OBJ)
    s.add_quad_light("QuadLight", *QUAD_LIGHT)
    names = []
    if form == "two":
        s.add_mesh(MESH, tri_v.reshape(-1, 9), (0.58, 0.58, 0.58))
        names.append(MESH)
    else:
        for i, f in enumerate(range(0, len(tri_v), 250)):
            s.add_mesh(f"{MESH}_{i:02d}", tri_v[f:f + 250].reshape(-1, 9), (0.58, 0.58, 0.58))
            names.append(f"{MESH}_{i:02d}")
    if material != "lambert":   # for WhittedIntegrator: the mesh re-tagged, and a point light inside the box
        s.add_point_light("PointLight", ws.translate(278.0, 400.0, 279.5), (1.0, 0.95, 0.9), 1.0e5)
        for nme in names:
            s.set_material(nme, material)
    s.flatten()
    s.camera = scenes.pinhole(camera, 60.0, w, h)
    s.integrator, s.max_depth = ("gi" if material == "lambert" else "whitted"), 3
    s.mesh_names = names
    return s


def spheres_irregular(w, h):
    """40 spheres: radii 8 * 2^(-k / 4) at x = 30 * 2^(-k / 3) along a line, every fifth one nested in
    its predecessor (same centre, half the radius), three concentric shells around the first, and
    the sphere light of scenes.spheres"""
    s = scenes.SceneBundle()
    k = 0
    prev = None
    for i in range(34):
        c = (30.0 * 2.0 ** (-i / 3.0) - 12.0, 2.0 * (i % 3), -14.0 - 0.7 * i)
        r = 8.0 * 2.0 ** (-i / 4.0)
        if i % 5 == 4:
            c, r = prev[0], 0.5 * prev[1]
        s.add_sphere(f"sphere_{k:02d}", c, r, (0.58, 0.58, 0.58))
        prev = (c, r)
        k += 1
    for j in range(3):
        s.add_sphere(f"sphere_{k:02d}", (18.0, 0.0, -14.0), 9.0 + j, (0.58, 0.58, 0.58))
        k += 1
    for j in range(3):
        s.add_sphere(f"sphere_{k:02d}", (-11.9 + 0.05 * j, 1.0, -40.0), 0.01 * (j + 1), (0.58, 0.58, 0.58))
        k += 1
    s.add_sphere_light("SphereLight", (0.0, 40.0, -20.0), 3.0, (30.0, 30.0, 30.0))
    s.flatten()
    s.camera = scenes.pinhole((1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 2.0, 6.0, 30.0, 1), 60.0, w, h)
    s.integrator, s.max_depth = "direct", 1
    return s


# name -> (octaves, diagonal).  The depths are those of the first build, build_bvh(..., kBvhMaxDepth), as
# tests/cpp/bvh_kat.cpp prints them for boxes(name); tests/test_bvh_build.py holds them to EDGES.
#   spiral_38d  one: depth 23, bvh_stack = kBvhStack, the deepest tree the binary walk takes (40 octaves
#               give 24); two: 4-wide depth 18, 3 * 18 + 1 > kBvh4Stack: refused before build_bvh_fit
#   spiral_22x  two: 4-wide depth 15, bvh4_stack = 46 of 48, the deepest first build the 4-wide walk takes
#   spiral_30d  one: depth 20; two: 4-wide depth 17: refused before build_bvh_fit
#   spiral_50d  depth 26: refused in both forms before build_bvh_fit
SPIRALS = {"spiral_38d": (38, True), "spiral_22x": (22, False), "spiral_30d": (30, True), "spiral_50d": (50, True)}
# case -> what the first build must reach ("depth" / "depth4") and whether it fits the walks' stacks
EDGES = {
    "spiral_38d-one": dict(depth=23, fits=True), "spiral_38d-two": dict(depth=23, depth4=18, fits=False),
    "spiral_22x-two": dict(depth4=15, fits=True),
    "spiral_30d-one": dict(depth=20, fits=True), "spiral_30d-two": dict(depth4=17, fits=False),
    "spiral_50d-one": dict(depth=26, fits=False), "spiral_50d-two": dict(depth=26, fits=False),
    "counts_63-two": dict(nodes=63, fits=True), "counts_64-two": dict(nodes=64, fits=True),
    "counts_65-two": dict(nodes=65, fits=True), "one_leaf-two": dict(nodes=1, depth=1, fits=True),
    "allcounts_63-one": dict(nodes=63, fits=True), "allcounts_64-one": dict(nodes=64, fits=True),
    "allcounts_65-one": dict(nodes=65, fits=True),
}


@functools.lru_cache(maxsize=None)
def triangles(family):
    """(vertices [n, 3, 3], kind [n]: 0 ordinary, 1 sliver, 2 collinear, 3 zero edge) of a family"""
    if family in SPIRALS:
        v = spiral_triangles(*SPIRALS[family])
    elif family == "concentric":
        v = concentric_triangles()
    elif family == "clumps":
        return clump_triangles()
    elif family.startswith("counts_"):
        n = STRIP_FOR_NODES[int(family[7:])]
        v = with_zero_edge(strip_triangles(n), N_SPIRAL)
    elif family.startswith("allcounts_"):
        v = with_zero_edge(strip_triangles(STRIP_FOR_ALL_NODES[int(family[10:])]), N_SPIRAL)
    elif family == "one_leaf":
        v = with_zero_edge(corner_triangles([[300.0, 380.0, 200.0], [200.0, 400.0, 300.0], [100.0, 360.0, 400.0]],
                                            [60.0, 80.0, 100.0]), N_SPIRAL)
    else:
        raise KeyError(family)
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    kind = np.where(np.all(e1 == 0, axis=1) | np.all(e2 == 0, axis=1), 3, 0)
    return v, kind


FAMILIES = tuple(SPIRALS) + ("concentric", "clumps", "counts_63", "counts_64", "counts_65", "one_leaf",
                            "allcounts_63", "allcounts_64", "allcounts_65")
# A node-count strip is tuned to one form.  counts_N and one_leaf: the mesh's own tree, which the
# kernels that walk the binary tree of a two-level scene read (k_whitted_bvh, k_aov_bvh: queries and
# the path integrators walk that scene's 4-wide form, of about 20 nodes).  allcounts_N: the one tree of
# the whole scene, which every kernel walks as a binary tree (k_trace_bvh for queries).
FORMS = {f: (("two",) if f.startswith("counts_") or f == "one_leaf" else ("one",) if f.startswith("allcounts_")
             else ("one", "two")) for f in FAMILIES}
CASES = tuple(f"{f}-{form}" for f in FAMILIES for form in FORMS[f])
# the cases around kBvhTopNodes whose binary tree a render walks
TOP_CASES = ("counts_63-two", "counts_64-two", "counts_65-two", "one_leaf-two",
             "allcounts_63-one", "allcounts_64-one", "allcounts_65-one")
W, H = 24, 18


@functools.lru_cache(maxsize=None)
def scene(name, material="lambert"):
    """the scene of CASES' `name` ("family-form") or "spheres_irregular", built once"""
    if name == "spheres_irregular":
        return spheres_irregular(W, H)
    family, form = name.rsplit("-", 1)
    # the spirals from their deep end; the strips and the one-leaf mesh from the front of the box
    camera = DEEP_C2W if family in SPIRALS else STRIP_C2W
    return cornell_with(triangles(family)[0], form, W, H, material, camera)


@functools.lru_cache(maxsize=None)
def culls(name):
    return Culls(scene(name))


def mesh_triangles(name):
    """per triangle of the mesh, in the family's order: its index in the scene's packed order (the
    order of Culls and of the device), whatever place the host scene gave the mesh's objects"""
    s, c = scene(name), culls(name)
    names = s.object_names()
    out = []
    for nme in s.mesh_names:
        k = names.index(nme)
        out += list(range(c.obj_first[k], c.obj_first[k] + c.mesh_count[k]))
    return np.asarray(out, int)


def boxes(name):
    """(box minima [n, 3], maxima, margin, two_level) of the triangles build_tri_bvh gives the build, in
    its order"""
    c = culls(name)
    assert c.bvh
    big = np.flatnonzero(c.tri_in_bvh)
    return c.t_lo[big], c.t_hi[big], F(c.pad_bvh), bool(c.two_level)


def sphere_boxes(name="spheres_irregular"):
    c = culls(name)
    assert c.sphere_bvh
    return c.s_lo, c.s_hi, F(c.pad_bvh), False


def write_boxes(path, lo, hi, margin, two_level, leaf_max=LEAF_TRI):
    with open(path, "wb") as f:
        f.write(struct.pack("<iiif", len(lo), leaf_max, int(two_level), float(margin)))
        f.write(np.ascontiguousarray(lo, F).tobytes())
        f.write(np.ascontiguousarray(hi, F).tobytes())


# ------------------------------------------------------------------ the host program ----
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xraytracer_amd", "csrc")


def constant(header, name):
    """the integer a header of csrc gives `name` (constexpr or #define)"""
    with open(os.path.join(CSRC, header)) as f:
        m = re.search(rf"\b{name}\s*=?\s*(\d+)", f.read())
    assert m, name
    return int(m.group(1))


def limits():
    return dict(KAT_MAX_DEPTH=constant("wavefront.h", "kBvhMaxDepth"), KAT_STACK=constant("wavefront.h", "kBvhStack"),
                KAT_STACK4=constant("wavefront.h", "kBvh4Stack"))


def box_files(directory, names=None):
    """the box files of the named cases (default: every case and the sphere scene), written to directory"""
    files = []
    for name in (CASES + ("spheres_irregular",) if names is None else names):
        files.append(os.path.join(str(directory), name))
        if name == "spheres_irregular":
            write_boxes(files[-1], *sphere_boxes(), leaf_max=4)   # wavefront.h kBvhLeaf
        else:
            write_boxes(files[-1], *boxes(name))
    return files


def run_program(directory, files, flags=()):
    """compile tests/cpp/bvh_kat.cpp with host/bvh.cpp (g++, the library's own floating-point flags) and
    run it once over the files: {input name: {field: text}} of the records it prints before its "ok" line"""
    exe = os.path.join(str(directory), "bvh_kat")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-ffp-contract=off", *flags,
                           *[f"-D{k}={v}" for k, v in limits().items()], "-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "bvh_kat.cpp"), os.path.join(CSRC, "host", "bvh.cpp")])
    run = subprocess.run([exe, *files], capture_output=True, text=True)
    lines = run.stdout.strip().splitlines()
    assert run.returncode == 0 and lines and lines[-1] == "ok", (run.returncode, lines[-3:], run.stderr[-2000:])
    return {ln.split()[0]: dict(kv.split("=") for kv in ln.split()[1:]) for ln in lines[:-1]}


# ------------------------------------------------------------------ rays ----
N_RAYS = 3000


def hittable(v):
    """triangles a unit direction can hit: |det| = |e1 . (d x e2)| reaches FLT_EPSILON, i.e. twice the
    area does; collinear and zero-edge triangles never do"""
    e1, e2 = (v[:, 1] - v[:, 0]).astype(np.float64), (v[:, 2] - v[:, 0]).astype(np.float64)
    return np.linalg.norm(np.cross(e1, e2), axis=1) > 4.0 * np.finfo(F).eps


@functools.lru_cache(maxsize=None)
def rays(name):
    """[N_RAYS, 6] float32 and tmax [N_RAYS] for the occluded query.  Thirds: from the deep end of the
    mesh (the smallest triangles; for a spiral the origin) outward; from outside the box at the
    triangles that can be hit; random over four times the box, with axis-parallel components."""
    rng = np.random.default_rng(sum(name.encode()))
    n = N_RAYS // 3
    if name == "spheres_irregular":
        sp = np.ctypeslib.as_array(scene(name).desc.spheres, shape=(scene(name).desc.n_spheres * 4,)).reshape(-1, 4)
        cen, size = sp[:, :3].astype(np.float64), np.abs(sp[:, 3]).astype(np.float64)
        lo, hi, outside = np.array([-40.0, -20.0, -70.0]), np.array([50.0, 40.0, 20.0]), np.array([2.0, 6.0, 30.0])
        can = np.ones(len(sp), bool)
    else:
        v = triangles(name.rsplit("-", 1)[0])[0]
        cen, size = v.mean(axis=1).astype(np.float64), np.ptp(v, axis=1).max(axis=1).astype(np.float64)
        lo, hi, outside = np.array([-560.0, -550.0, -1100.0]), np.array([1100.0, 1100.0, 1100.0]), np.array([278.0, 274.4, -750.0])
        can = hittable(v)
    deep = cen[np.argmin(np.where(can, size, np.inf))]          # the smallest triangle that can be hit
    # 1: from around the deep end, outward to triangles that can be hit, so the hits are stacked behind
    # the nearest and the walk starts where the tree is deepest
    tgt = cen[rng.choice(np.flatnonzero(can), n)]
    o1 = deep + rng.normal(size=(n, 3)) * 1e-3 * np.maximum(np.abs(deep), 1.0)
    o1[::4] = deep * 0.5
    d1 = tgt - o1 + rng.normal(size=(n, 3)) * 0.02 * np.linalg.norm(tgt - o1, axis=1, keepdims=True)
    # 2: at the triangles that can be hit, from outside
    tgt = cen[rng.choice(np.flatnonzero(can), n)]
    o2 = outside + rng.normal(size=(n, 3)) * 40.0
    d2 = tgt - o2
    d2[::2] /= np.linalg.norm(d2[::2], axis=1, keepdims=True)
    # 3: random (tests/test_gpu_query.py random_rays)
    n3 = N_RAYS - 2 * n
    o3 = rng.uniform(lo, hi, (n3, 3))
    d3 = rng.normal(size=(n3, 3))
    d3[::3] /= np.linalg.norm(d3[::3], axis=1, keepdims=True)
    d3[7::11, 1] = 0.0
    d3[5::13, 0] = 0.0
    r = np.concatenate([np.concatenate([o1, d1], axis=1), np.concatenate([o2, d2], axis=1), np.concatenate([o3, d3], axis=1)]).astype(F)
    bad = np.all(r[:, 3:] == 0, axis=1)
    r[bad, 3:] = (1.0, 0.0, 0.0)
    # occluded: the limit below and above the distance to the target, in the ray's own parameter
    tmax = rng.uniform(0.0, 2.0, N_RAYS).astype(F)
    tmax[2 * n:] = rng.uniform(0.0, 800.0, n3).astype(F)
    # (a ray with a unit direction measures length, the others reach their target at t = 1)
    tmax[n:2 * n:2] = (tmax[n:2 * n:2] * np.linalg.norm(tgt - o2, axis=1)[::2]).astype(F)
    r.setflags(write=False)
    tmax.setflags(write=False)
    return r, tmax


@functools.lru_cache(maxsize=None)
def reference(name):
    """(closest hits, occluded flags) of the oracle for rays(name); computed once"""
    r, tmax = rays(name)
    s = scene(name)
    return pyoracle.query(s, r), [h.hit for h in pyoracle.query(s, r, tmax=tmax, occluded=True)]
