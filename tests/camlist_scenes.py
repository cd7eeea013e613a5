"""Scenes for the camera-list tests (tests/test_camlist_restatement.py on the CPU,
tests/test_gpu_camlist.py on the device) — a test helper, not a test file.

CASES names every scene whose lists are checked: the ones of tests/elide_scenes.py and the
adversarial ones built here, each for one claim of the lists (tests/camlist_restatement.py).
Every scene is GIIntegrator(3) with one area light, at most 64 triangles and 32 objects, so the
device takes the speculative merged schedule; neighbouring triangles belong to objects of
different albedo, so a wrong winner changes the frame.  What a scene is for — the pixels of
its class that its lists must hold — is stated here once, as `need` (minimum pixel counts per
class of camlist_restatement.classes) and `holds` (assertions over the restated lists, which
the device's are required to equal); `check_classes` applies both.  They are conditions that
keep a test from idling, not measurements: the floors follow from the geometry (a full-frame
triangle covers every pixel, the box fills half the Cornell frame), and lists that give far
fewer are wrong lists.

The adversarial scenes use elide_scenes.eye_scene (the eye at the origin looking down -z) and
name their geometry by pixel coordinates through elide_scenes.at.  Triangle indices matter
here (the lists are bit masks over them), and the host scene keeps its objects in a hash map:
`ordered` builds a scene whose objects come out of the flattening in the order given.
"""
import collections

import numpy as np

from xraytracer_amd import scenes

import camlist_restatement as cr
import elide_scenes as es

W, H = 32, 24   # the adversarial scenes' frame


def ordered(s, parts):
    """Add `parts` — ("mesh", triangles, albedo), ("quad_light", v0, v1, v2, Le) or
    ("triangle_light", v0, v1, v2, Le) — to the empty scene s so that they are its objects 0,
    1, ... after flattening, and flatten it.  The order a hash map iterates in follows from the
    keys and the order they were inserted in alone, so a first scene of placeholders under the
    same names shows which name comes out where."""
    names = [f"part_{k:02d}" for k in range(len(parts))]
    probe = scenes.SceneBundle()
    for n in names:
        probe.add_mesh(n, [((0, 0, 0), (1, 0, 0), (0, 1, 0))], (0.5, 0.5, 0.5))
    probe.flatten()
    order = probe.object_names()
    assert sorted(order) == names, order
    for n in names:
        kind, *args = parts[order.index(n)]
        {"mesh": s.add_mesh, "quad_light": s.add_quad_light, "triangle_light": s.add_triangle_light}[kind](n, *args)
    s.flatten()
    assert s.object_names() == order, (s.object_names(), order)
    first = [s.desc.objects[k].first for k in range(s.desc.n_objects)]
    assert first == sorted(first), first
    return s


def px(x, y, z):
    """the world point the continuous pixel coordinate (x, y) of the W x H frame sees at depth z"""
    return es.at(W, H, x, y, z)


def full_frame(z, flip=False):
    """a triangle at depth z over the whole frame and a margin round it; flip: wound the other
    way, its normal pointing away from the eye"""
    a, b, c = px(-4.0, -4.0, z), px(2.0 * W + 8.0, -4.0, z), px(-4.0, 2.0 * H + 8.0, z)
    return (a, b, c) if flip else (a, c, b)


# a quad light above the view, facing down (no camera ray sees it)
LAMP = ("quad_light", (-2.0, 3.0, -4.0), (-2.0, 3.0, -6.0), (2.0, 3.0, -4.0), (20.0, 20.0, 20.0))
RED, GREEN, BLUE, GREY = (0.8, 0.2, 0.2), (0.2, 0.8, 0.2), (0.2, 0.2, 0.8), (0.6, 0.6, 0.6)


def stacked():
    """Three full-frame triangles: 0 the far one (0.5 behind the front one: culled), 1 the front
    one at depth 10, 2 the one 1e-3 behind it (inside the cull's margin of 1e-4 (10 + 10 + ...):
    it stays listed).  The far one comes first, so the cull does not follow the index order."""
    return ordered(es.eye_scene(W, H), [("mesh", [full_frame(10.5)], RED), ("mesh", [full_frame(10.0)], GREEN),
                                        ("mesh", [full_frame(10.001)], BLUE), LAMP])


def stacked_holds(L):
    inside = L.cover[:, 1]
    assert inside.all()
    assert not L.keep[inside, 0].any() and L.mask[inside, 0].all()   # the far one: listed, then culled
    assert L.keep[inside, 1].all() and L.keep[inside, 2].all()       # the near pair stays
    assert np.all(L.covering == -1)


def coincident():
    """Two identical full-frame triangles (0, 1): both cover, neither lies beyond the other, so
    neither is culled and no shortcut is taken; the strict t < best keeps the lower index."""
    return ordered(es.eye_scene(W, H), [("mesh", [full_frame(10.0)], RED), ("mesh", [full_frame(10.0)], GREEN), LAMP])


def coincident_holds(L):
    assert np.all(L.covering == -1) and np.array_equal(L.mask, L.keep)
    assert (L.keep[:, 0] & L.keep[:, 1]).sum() >= W * H


def crossing():
    """A full-frame triangle (0) and a triangle (1) that passes through its plane inside the
    view, from depth 8 on the left to depth 12 on the right: never culled."""
    tri = (px(6.0, 4.0, 8.0), px(16.0, 21.0, 10.0), px(27.0, 5.0, 12.0))
    return ordered(es.eye_scene(W, H), [("mesh", [full_frame(10.0)], RED), ("mesh", [tri], GREEN), LAMP])


def crossing_holds(L):
    assert np.array_equal(L.mask[:, 1], L.keep[:, 1]) and L.keep[:, 1].sum() >= 100
    assert np.all(L.covering[L.keep[:, 1]] == -1)


MARGIN_COLS = (6, 25)    # the column the 5e-4 edge runs along, and the column of the 2e-3 one
MARGIN_ROWS = (slice(0, 10), slice(13, 24))
MARGIN_SPAN = 40.0       # pixels along the triangles' u axis: 5e-4 is 0.02 pixel


def margin_edge():
    """Two triangles at depth 10, parallel to the image plane (their barycentrics are affine in
    the pixel coordinates).  Triangle 0's u = 0 edge runs down the frame 5e-4 outside the widened
    left corners (x = col - 0.01) of column MARGIN_COLS[0]: every camera ray of those pixels
    hits it, and yet it does not cover them by the margin of 1e-3.  Triangle 1 is its mirror
    image lower in the frame, its edge 2e-3 outside the right corners of column MARGIN_COLS[1]:
    it covers them."""
    x0 = MARGIN_COLS[0] - 0.01 - 5e-4 * MARGIN_SPAN
    x1 = MARGIN_COLS[1] + 1.01 + 2e-3 * MARGIN_SPAN
    a = (px(x0, -2.0, 10.0), px(x0 + MARGIN_SPAN, -2.0, 10.0), px(x0, 12.0, 10.0))
    b = (px(x1, 12.5, 10.0), px(x1 - MARGIN_SPAN, 12.5, 10.0), px(x1, 26.5, 10.0))
    return ordered(es.eye_scene(W, H), [("mesh", [a], RED), ("mesh", [b], GREEN), LAMP])


def margin_pixels():
    """the slots of the two columns' pixels: (5e-4 inside, 2e-3 inside)"""
    rows = np.arange(H)
    return tuple(rows[r] * W + c for r, c in zip(MARGIN_ROWS, MARGIN_COLS))


def margin_edge_holds(L):
    near, far = margin_pixels()
    assert L.keep[near, 0].all() and not L.cover[near, 0].any() and np.all(L.covering[near] == -1)
    assert np.all(L.covering[far] == 1)
    assert np.all(L.covering[near + 1] == 0)   # one column further in it covers


GRAZE_W, GRAZE_H, GRAZE_ROW = 64, 16, 8


def grazing():
    """A triangle in a plane that passes 0.01 below the eye and rises by 1e-3 per unit of depth,
    in a 64 x 16 frame whose pixels are 1.03 degrees high: the camera rays of row GRAZE_ROW, the
    first below the frame's middle, meet it at 0.04 (top corners) to 1.1 degrees (bottom corners),
    between 0.5 and 16 away — its determinant is small against |e1| |e2| |D|."""
    plane = lambda x, z: (x, -0.01 + 1e-3 * z, -z)
    tri = (plane(-60.0, 60.0), plane(0.0, -0.5), plane(60.0, 60.0))
    return ordered(es.eye_scene(GRAZE_W, GRAZE_H), [("mesh", [tri], GREY), LAMP])


def grazing_holds(L):
    row = L.covering[GRAZE_ROW * GRAZE_W:(GRAZE_ROW + 1) * GRAZE_W]
    assert np.all(row == 0), row


def back_facing():
    """A full-frame triangle (1) whose normal points away from the eye, a triangle 2 behind it
    (0: culled) and a smaller one 2 in front of it (2: stays, and is hit first where it lies)."""
    front = (px(8.0, 5.0, 8.0), px(14.0, 19.0, 8.0), px(25.0, 7.0, 8.0))
    return ordered(es.eye_scene(W, H), [("mesh", [full_frame(12.0)], RED), ("mesh", [full_frame(10.0, flip=True)], GREEN),
                                        ("mesh", [front], BLUE), LAMP])


def back_facing_holds(L):
    inside = L.cover[:, 1]
    assert inside.all()
    assert not L.keep[inside, 0].any() and L.mask[inside, 0].all()
    assert np.array_equal(L.mask[:, 2], L.keep[:, 2]) and L.keep[:, 2].sum() >= 50


def emissive_cover():
    """The light itself — a triangle light facing the eye over the frame's upper left (0) —
    covers pixels, with a Lambert full-frame triangle 2 beyond it (1: culled there) and a floor."""
    s = es.eye_scene(W, H)
    light = ("triangle_light", px(-6.0, -6.0, 10.0), px(-6.0, 34.0, 10.0), px(34.0, -6.0, 10.0), (6.0, 5.0, 4.0))
    a, b = px(-4.0, 0.7 * H, 6.0), px(W + 4.0, 0.7 * H, 6.0)
    c, d = px(W + 4.0, 0.95 * H, 9.0), px(-4.0, 0.95 * H, 9.0)
    return ordered(s, [light, ("mesh", [full_frame(12.0)], RED), ("mesh", [(a, b, c), (a, c, d)], GREEN)])


def emissive_cover_holds(L):
    lit = L.covering == 0
    assert lit.sum() >= 100 and L.mask[lit, 1].all() and not L.keep[lit, 1].any()


def cornell_scaled(k, width=64, height=48):
    """the Cornell box and its camera multiplied by k: the same picture; of the lists' margins
    only the side planes' has an absolute part"""
    src = scenes.cornell(width, height)
    tris, d = src.triangles(), src.desc
    s = scenes.SceneBundle()
    for q in range(d.n_objects):
        o = d.objects[q]
        if o.light < 0:
            s.add_mesh(f"mesh_{q:02d}", tris[o.first:o.first + o.count] * np.float32(k), tuple(o.albedo))
    sc = lambda v: tuple(float(x) * k for x in v)
    s.add_quad_light("QuadLight", sc((343.0, 548.0, 227.0)), sc((343.0, 548.0, 332.0)), sc((213.0, 548.0, 227.0)),
                     (25.0, 25.0, 25.0))
    s.flatten()
    c2w = np.asarray(scenes.CORNELL_C2W, np.float64)
    c2w[12:15] *= k
    s.camera = scenes.pinhole(c2w, 60.0, width, height)
    return s


TILE_W, TILE_H = 4.0, 6.0   # pixels


def tiles_64(extra=False):
    """Exactly 64 triangles in four objects: 0 a triangle light above the view, 1-31 and 32-62
    two meshes that tile a wall at depth 10 with 31 quads of 4 x 6 pixels (column by column, 0.3
    pixel off the pixel grid; quad q is triangles 1 + 2 q and 2 + 2 q, so 31 and 32 are the
    halves of quad 15, in different meshes), 63 a triangle at depth 8 over the frame's right
    half, which hides the wall there.  extra: one more triangle behind the wall, 65 in all."""
    tris = []
    for q in range(31):
        x, y = (q // 4) * TILE_W + 0.3, (q % 4) * TILE_H + 0.3
        a, b, c, d = px(x, y, 10.0), px(x + TILE_W, y, 10.0), px(x + TILE_W, y + TILE_H, 10.0), px(x, y + TILE_H, 10.0)
        tris += [(a, c, b), (a, d, c)]
    big = (px(16.7, -4.0, 8.0), px(16.7, 40.0, 8.0), px(60.7, -4.0, 8.0))
    parts = [("triangle_light", (-2.0, 3.0, -4.0), (-2.0, 3.0, -6.0), (2.0, 3.0, -4.0), (30.0, 30.0, 30.0)),
             ("mesh", tris[:31], RED), ("mesh", tris[31:], GREEN), ("mesh", [big], BLUE)]
    if extra:
        parts.append(("mesh", [full_frame(14.0)], GREY))
    s = ordered(es.eye_scene(W, H), parts)
    assert s.desc.n_tris == (65 if extra else 64)
    return s


def tiles_64_holds(L):
    assert (L.covering == 63).sum() >= 100
    assert (L.keep[:, 31] & L.keep[:, 32]).sum() >= 4      # the quad's diagonal crosses these pixels
    assert np.all(L.words[L.covering == 63, 1] == 0x80000000) and np.all(L.words[L.covering == 63, 0] == 0)


Case = collections.namedtuple("Case", "build width height need holds")
CORNELL_NEED = dict(covered=500, multi=300, culled=100, empty=1000)
BOTH = dict(empty=1)   # the elide scenes: what they are for is tests/test_camlist_restatement.py's older half


def _elide(build, w=W, h=H, need=BOTH):
    return Case(build, w, h, need, None)


CASES = {
    "cornell": _elide(lambda: scenes.cornell(64, 48), 64, 48, CORNELL_NEED),
    "cornell_shifted": _elide(lambda: es.cornell_shifted(64, 48), 64, 48, CORNELL_NEED),
    **{f"random_{seed:02d}": _elide(lambda seed=seed: es.random_scene(seed)) for seed in range(20)},
    # (random scene 7 is one triangle some 20 pixels large: it covers whole pixels only in a finer frame)
    "random_07": _elide(lambda: es.random_scene(7, 64, 48), 64, 48),
    **{name: _elide(fn) for name, fn in es.SILHOUETTES.items()},
    "stacked": Case(stacked, W, H, dict(multi=W * H, culled=W * H), stacked_holds),
    "coincident": Case(coincident, W, H, dict(tied=W * H), coincident_holds),
    "crossing": Case(crossing, W, H, dict(covered=8, multi=100), crossing_holds),
    "margin_edge": Case(margin_edge, W, H, dict(single=10, covered=11), margin_edge_holds),
    "grazing": Case(grazing, GRAZE_W, GRAZE_H, dict(covered=GRAZE_W, empty=8), grazing_holds),
    "back_facing": Case(back_facing, W, H, dict(culled=W * H, covered=8, multi=50), back_facing_holds),
    "emissive_cover": Case(emissive_cover, W, H, dict(covered=100, culled=100, multi=8), emissive_cover_holds),
    "cornell_small": _elide(lambda: cornell_scaled(1e-3), 64, 48, CORNELL_NEED),
    "cornell_large": _elide(lambda: cornell_scaled(1e3), 64, 48, CORNELL_NEED),
    "tiles_64": Case(tiles_64, W, H, dict(covered=100, multi=8, culled=100), tiles_64_holds),
}
ADVERSARIAL = ("stacked", "coincident", "crossing", "margin_edge", "grazing", "back_facing", "emissive_cover",
               "cornell_small", "cornell_large", "tiles_64")


def check_classes(name, lists):
    """the restated lists (camlist_restatement.camera_lists) hold the pixels scene `name` exists
    for, and covered or multi-triangle pixels whatever it is for; returns the classes' pixel counts"""
    case = CASES[name]
    count = {k: int(v.sum()) for k, v in cr.classes(lists).items()}
    assert count["covered"] + count["multi"] > 0, (name, count)
    for k, floor in case.need.items():
        assert count[k] >= floor, (name, k, count[k], floor)
    if case.holds:
        case.holds(lists)
    return count
