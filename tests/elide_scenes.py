"""Scenes for the empty-pixel tests (tests/test_camlist_restatement.py on the CPU,
tests/test_gpu_elide.py on the device) — a test helper, not a test file.  tests/camlist_scenes.py
adds them, and scenes of its own built on `eye_scene` and `at`, to the camera-list tests.

Every scene is a handful of triangles under GIIntegrator(3) with one area light, so the device
renders it in the merged schedule.  `eye_scene` puts the camera at the origin looking down -z
(FOV 60); `at(W, H, x, y, z)` is then the world point that the continuous pixel coordinate
(x, y) — column x, row y, the pixel (i, j) covering [j, j + 1) x [i, i + 1) — sees at depth z.
"""
import numpy as np

from xraytracer_amd import scenes

EYE_C2W = (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1)
AWAY_C2W = (1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, 0, 278, 274.4, -750.0, 1)   # the Cornell camera, turned round
SHIFT = 1e4


def at(width, height, x, y, z=10.0):
    scale = np.tan(np.deg2rad(30.0))
    aspect = width / height
    return ((2.0 * x / width - 1.0) * scale * z, (1.0 - 2.0 * y / height) * scale / aspect * z, -z)


def eye_scene(width, height):
    s = scenes.SceneBundle()
    s.camera = scenes.pinhole(EYE_C2W, 60.0, width, height)
    s.integrator, s.max_depth = "gi", 3
    return s


def cornell_away(width, height):
    """the Cornell box behind the camera: no camera ray hits anything"""
    s = scenes.cornell(width, height)
    s.camera = scenes.pinhole(AWAY_C2W, 60.0, width, height)
    return s


def cornell_shifted(width, height, shift=SHIFT):
    """the Cornell box and its camera translated by `shift` on every axis: the same picture
    from coordinates whose float32 spacing is 1e-3"""
    src = scenes.cornell(width, height)
    tris = src.triangles()
    s = scenes.SceneBundle()
    d = src.desc
    for k in range(d.n_objects):
        o = d.objects[k]
        if o.light >= 0:
            continue
        s.add_mesh(f"mesh_{k:02d}", tris[o.first:o.first + o.count] + np.float32(shift), tuple(o.albedo))
    sh = lambda v: tuple(float(x) + shift for x in v)
    s.add_quad_light("QuadLight", sh((343.0, 548.0, 227.0)), sh((343.0, 548.0, 332.0)), sh((213.0, 548.0, 227.0)),
                     (25.0, 25.0, 25.0))
    s.flatten()
    c2w = np.asarray(scenes.CORNELL_C2W, np.float64)
    c2w[12:15] += shift
    s.camera = scenes.pinhole(c2w, 60.0, width, height)
    return s


def floor(s, width, height):
    """a Lambert quad across the lower third of the frame, at depth 10 .. 20"""
    a, b = at(width, height, -4.0, 0.7 * height, 10.0), at(width, height, width + 4.0, 0.7 * height, 10.0)
    c, d = at(width, height, width + 4.0, 0.9 * height, 20.0), at(width, height, -4.0, 0.9 * height, 20.0)
    s.add_mesh("floor", [(a, b, c), (a, c, d)], (0.6, 0.5, 0.4))


QUARTER_PIXEL = (10, 13)   # (row, column)


def quarter_pixel(width=32, height=24):
    """an emissive triangle inside pixel QUARTER_PIXEL, about a fifth of its area, clear of the
    pixel's corners and of its centre; a Lambert floor below"""
    i, j = QUARTER_PIXEL
    s = eye_scene(width, height)
    s.add_triangle_light("speck", at(width, height, j + 0.53, i + 0.04), at(width, height, j + 0.53, i + 0.96),
                         at(width, height, j + 0.97, i + 0.50), (40.0, 30.0, 20.0))   # faces the eye
    floor(s, width, height)
    s.flatten()
    return s


def sliver(width=32, height=24):
    """an emissive strip 0.2 pixel wide from the frame's top left to its bottom right"""
    s = eye_scene(width, height)
    p0, p1 = np.array([-1.0, -0.6]), np.array([width + 1.0, height + 0.8])
    along = (p1 - p0) / np.linalg.norm(p1 - p0)
    perp = 0.2 * np.array([-along[1], along[0]])
    s.add_quad_light("strip", at(width, height, *p0), at(width, height, *(p0 + perp)), at(width, height, *p1),
                     (30.0, 30.0, 30.0))
    floor(s, width, height)
    s.flatten()
    return s


def edge_on(width=32, height=24):
    """a Lambert triangle 10 wide and 26 deep whose plane passes 0.02 above the eye: it projects
    onto a fraction of one pixel row; a quad light above it"""
    s = eye_scene(width, height)
    s.add_mesh("blade", [((-5.0, 0.02, -4.0), (5.0, 0.02, -4.0), (0.0, 0.05, -30.0))], (0.7, 0.7, 0.7))
    s.add_quad_light("lamp", (-2.0, 3.0, -8.0), (-2.0, 3.0, -12.0), (2.0, 3.0, -8.0), (20.0, 20.0, 20.0))   # faces down
    s.flatten()
    return s


def near_wall(width=32, height=24):
    """the eye 5e-4 from a Lambert wall that starts beside it (x = -5e-4, z from 0 to -20): the
    left half of the frame sees the wall from closer than 0.02, the right half nothing but part
    of a quad light — and no edge plane of the wall's triangles decides anything"""
    s = eye_scene(width, height)
    x = -5e-4
    a, b, c, d = (x, -2.0, 0.0), (x, -2.0, -20.0), (x, 2.0, -20.0), (x, 2.0, 0.0)
    s.add_mesh("wall", [(a, b, c), (a, c, d)], (0.6, 0.6, 0.6))
    s.add_quad_light("lamp", (3.0, -1.0, -6.0), (3.0, -1.0, -4.0), (3.0, 1.0, -6.0), (20.0, 20.0, 20.0))   # faces the wall
    s.flatten()
    return s


def random_scene(seed, width=32, height=24):
    """1 .. 12 triangles (the first one emissive) in the cube [-1.5, 1.5]^3, seen from a random
    point 5 .. 8 away with a random roll, looking at a point near the origin"""
    rng = np.random.default_rng(1000 + seed)
    n = int(rng.integers(1, 13))
    tris = rng.uniform(-1.5, 1.5, (n, 3, 3))
    s = scenes.SceneBundle()
    s.add_triangle_light("light", tuple(tris[0, 0]), tuple(tris[0, 1]), tuple(tris[0, 2]), (15.0, 15.0, 15.0))
    for k in range(1, n):
        s.add_mesh(f"tri_{k:02d}", [tris[k]], tuple(rng.uniform(0.2, 0.9, 3)))
    s.flatten()
    pos = rng.normal(size=3)
    pos *= rng.uniform(5.0, 8.0) / np.linalg.norm(pos)
    back = pos - rng.uniform(-0.5, 0.5, 3)      # camera z: away from the target
    back /= np.linalg.norm(back)
    up = rng.normal(size=3)
    right = np.cross(up, back)
    right /= np.linalg.norm(right)
    up = np.cross(back, right)
    c2w = np.zeros(16)
    c2w[0:3], c2w[4:7], c2w[8:11], c2w[12:15], c2w[15] = right, up, back, pos, 1.0
    s.camera = scenes.pinhole(c2w, 60.0, width, height)
    s.integrator, s.max_depth = "gi", 3
    return s


SILHOUETTES = {"quarter_pixel": quarter_pixel, "sliver": sliver, "edge_on": edge_on, "near_wall": near_wall}
