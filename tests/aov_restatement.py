"""The guide-buffer pass (xrt_render_aov) restated on the frozen oracle — a test helper, not a
test file, in the style of tests/whitted_restatement.py.

numpy float32 throughout, one operation per statement.  From oracle/pyoracle.py it takes the
per-pixel stream (``draws``, seed j + W*i), the camera ray (``orc_kat_camera``) and
Scene::intersect (``orc_query``, through whitted_restatement._query); albedo and material come
from ``scene.desc.objects``.  The reduction is the contract of include/xrt.h: every float channel
starts at +0.0f, takes every sample's value in sample order k = 0 .. spp - 1 (a miss adds
+0.0f), and is divided once by np.float32(spp); ``object`` is sample 0's.

CASES are the frames tests/test_gpu_aov.py compares with the device's, each restated once per
session (``reference``); tests/test_aov_restatement.py checks without a GPU that they reach
the situations the GPU test relies on.
"""
import ctypes as C
import functools

import numpy as np

import pyoracle
import whitted_bvh_scenes as wb
import whitted_restatement as wr
import whitted_scenes as ws
from xraytracer_amd import abi

F = np.float32
PLANES = abi.AOV_PLANES   # ("albedo", "normal", "depth", "alpha", "object")


def camera_rays(scene, width, height, spp, rows):
    """PinholeCamera::sampleRay for every sample of the pixels of `rows` (Src/renderer.cpp:35-47):
    sample k of pixel (i, j) takes words 2k, 2k + 1 of the stream seeded j + width * i.
    Returns (pixels [(i, j)], origins [n, spp, 3], directions [n, spp, 3])."""
    cam = pyoracle.camera(scene.camera)
    pix = [(i, j) for i in rows for j in range(width)]
    ro = np.zeros((len(pix), spp, 3), F)
    rd = np.zeros((len(pix), spp, 3), F)
    co, cd = np.zeros(3, F), np.zeros(3, F)
    lib = pyoracle.lib()
    for n, (i, j) in enumerate(pix):
        w = pyoracle.draws(j + width * i, 2 * spp)
        for k in range(spp):
            x = F(j) + w[2 * k]
            y = F(i) + w[2 * k + 1]
            u = F(x) / F(width)
            v = F(y) / F(height)
            lib.orc_kat_camera(C.byref(cam), C.c_float(u), C.c_float(v), pyoracle.fp(co), pyoracle.fp(cd))
            ro[n, k], rd[n, k] = co, cd
    return pix, ro, rd


def sample_values(scene, ro, rd):
    """one Scene::intersect per ray [S, 3]: (object [S] int32, values [S, 8] float32 = albedo.rgb,
    ns.xyz, t, 1 — all +0.0f on a miss)"""
    h = wr._query(scene, ro, rd)
    obj = h[:, 1].view(np.int32).copy()
    ns = h[:, 11:14]
    t = h[:, 3]
    n_obj = scene.desc.n_objects
    mats = np.array([scene.desc.objects[i].material for i in range(n_obj)] + [abi.XRT_MAT_NONE], np.int32)
    raw = np.array([scene.desc.objects[i].albedo[:] for i in range(n_obj)] + [(0, 0, 0)], F)
    val = np.zeros((len(obj), 8), F)
    hit = obj >= 0
    mat = mats[obj]   # obj -1 -> the appended NONE entry (unused)
    lam = hit & (mat == abi.XRT_MAT_LAMBERT)
    spec = hit & ((mat == abi.XRT_MAT_METAL) | (mat == abi.XRT_MAT_GLASS))
    val[lam, 0:3] = raw[obj[lam]]
    val[spec, 0:3] = F(1.0)
    val[hit, 3:6] = ns[hit]
    val[hit, 6] = t[hit]
    val[hit, 7] = F(1.0)
    return obj, val


def render(scene, width, height, spp, shard_index=0, shard_count=1):
    """(planes dict, counters dict, per-sample dict: obj [n, spp], val [n, spp, 8], ro, rd
    [n, spp, 3], pix [(i, j)]) over the rows y % shard_count == shard_index"""
    rows = [i for i in range(height) if i % shard_count == shard_index]
    pix, ro, rd = camera_rays(scene, width, height, spp, rows)
    obj, val = sample_values(scene, ro.reshape(-1, 3), rd.reshape(-1, 3))
    obj = obj.reshape(len(pix), spp)
    val = val.reshape(len(pix), spp, 8)
    acc = np.zeros((len(pix), 8), F)   # +0.0f
    for k in range(spp):               # in sample order; a miss adds +0.0f
        acc = acc + val[:, k]
    mean = acc / F(spp)                # one IEEE division
    planes = dict(albedo=np.zeros((height, width, 3), F), normal=np.zeros((height, width, 3), F),
                  depth=np.zeros((height, width), F), alpha=np.zeros((height, width), F),
                  object=np.full((height, width), -1, np.int32))
    for n, (i, j) in enumerate(pix):
        planes["albedo"][i, j] = mean[n, 0:3]
        planes["normal"][i, j] = mean[n, 3:6]
        planes["depth"][i, j] = mean[n, 6]
        planes["alpha"][i, j] = mean[n, 7]
        planes["object"][i, j] = obj[n, 0]
    samples = len(pix) * spp
    cnt = dict(samples=samples, segments=samples, shadow_rays=0, draws=2 * samples, rejected=0, path_slots=len(pix),
               schedule=abi.XRT_SCHED_AOV)
    return planes, cnt, dict(obj=obj, val=val, ro=ro, rd=rd, pix=pix)


COUNTERS = ("samples", "segments", "shadow_rays", "draws", "rejected", "path_slots", "schedule")

# scene kinds over the LDS-resident scene (k_aov), 24 x 18 at 2 spp: the builders of ws.CASES
LDS_KINDS = ("cornell_tri", "spheres_small", "spheres_bvh", "medium_box", "cornell_emitter", "mirrors_3", "glass_3")
# triangle scenes beyond LDS (k_aov_bvh), wb.CASES: two-level, one-level, ties across and inside the BVH
BVH_KINDS = ("glass", "big_meshes", "tie_before", "tie_after", "twins")
# window and ring-chunk edges of the ordered sum, on example(8, 6): below, at and above one
# 64-sample window, two windows and a bit, and past one 624-word block (sample 312)
EDGE_SPP = (1, 63, 64, 65, 130, 330)


def _ws_scene(name):
    # ws.CASES renders glass at 16 x 12; the guide cases are all 24 x 18 (the camera's aspect follows)
    return ws.glass(24, 18) if name == "glass_3" else ws.scene(name)


# name -> (scene builder, width, height, spp, render keywords)
CASES = {}
for _n in LDS_KINDS:
    CASES[_n] = (functools.partial(_ws_scene, _n), 24, 18, 2, {})
for _n in BVH_KINDS:
    CASES["bvh_" + _n] = (functools.partial(wb.scene, _n), 24, 18, 2, {})
for _s in EDGE_SPP:
    CASES[f"edge_{_s}"] = (functools.partial(ws.example, 8, 6), 8, 6, _s, {})
CASES["example"] = (functools.partial(ws.example, 48, 36), 48, 36, 3, {})
CASES["example_shard"] = (functools.partial(ws.example, 48, 36), 48, 36, 3, dict(shard_index=1, shard_count=3))


@functools.lru_cache(maxsize=None)
def scene(name):
    return CASES[name][0]()


@functools.lru_cache(maxsize=None)
def reference(name):
    """(planes, counters, per-sample record) of the restatement for CASES[name]; computed once and
    read-only"""
    _, w, h, spp, kw = CASES[name]
    planes, cnt, per = render(scene(name), w, h, spp, **kw)
    for a in planes.values():
        a.setflags(write=False)
    return planes, cnt, per
