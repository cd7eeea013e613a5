#!/usr/bin/env python3
"""tools/whitted_bench.py — time WhittedIntegrator renders on one GPU and print one JSON object.

  --scene example   scenes.example at 780 x 585, 16 and 1024 spp (the LDS kernel, k_whitted):
                    what profiles/whitted_example*.json record
  --scene mesh      scenes.cornell_spheremesh (160 x 160 SphereMesh, 51,200 triangles) with the
                    mesh tagged glass and a point light inside, 800 x 600, 64 spp, max_depth 3,
                    XRT_FLAG_WHITTED_BVH (k_whitted_bvh): profiles/whitted_bvh_c4.json

One warm-up render per shape, then --runs timed renders with XRT_FLAG_TIMING; wall time is the
library's clock around the render call (it ends in a stream synchronise), kernel time the HIP
events around the one XRT_K_STEP launch.  The library is the one abi.py loads (XRT_LIB selects
another build of the same ABI), so two builds are compared by running this twice."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from xraytracer_amd import abi, scenes   # noqa: E402
from xraytracer_amd.renderer import HipRenderer   # noqa: E402

SCHED = {abi.XRT_SCHED_WHITTED: "whitted", abi.XRT_SCHED_WHITTED_BVH: "whitted_bvh", abi.XRT_SCHED_PIXEL: "pixel"}
TRANSLATE = (1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0)


def timed(scene, w, h, spp, runs, **kw):
    r = HipRenderer(spp)
    try:
        r.render(scene, w, h, timing=True, **kw)   # warm-up: code objects, buffers, the upload
        wall, step = [], []
        for _ in range(runs):
            r.render(scene, w, h, timing=True, **kw)
            wall.append(r.stats.wall_ms)
            step.append(r.stats.kernel_ms[abi.XRT_K_STEP])
        st = r.stats
        wm, sm = statistics.median(wall), statistics.median(step)
        return dict(integrator=kw.get("integrator") or scene.integrator, width=w, height=h, spp=spp,
                    max_depth=kw.get("max_depth", scene.max_depth), schedule=SCHED.get(int(st.schedule), int(st.schedule)),
                    samples=int(st.samples), wall_ms=wall, wall_ms_median=wm, kernel_ms_step=step, kernel_ms_step_median=sm,
                    msamples_per_s=st.samples / wm / 1e3, msamples_per_s_kernel=st.samples / sm / 1e3,
                    segments=int(st.segments), shadow_rays=int(st.shadow_rays), whit_rays=int(st.whit_rays),
                    whit_depth_cut=int(st.whit_depth_cut), whit_refract=int(st.whit_refract), whit_tir=int(st.whit_tir))
    finally:
        r.close()


def mesh_scene(w, h, n):
    s = scenes.cornell_spheremesh(w, h, n_theta=n, n_phi=n)
    s.add_point_light("PointLight", TRANSLATE + (278.0, 400.0, 279.5, 1), (1.0, 0.95, 0.9), 1.0e5)
    s.set_material("sphere_mesh", "glass")
    s.flatten()
    s.integrator, s.max_depth = "whitted", 3
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scene", choices=("example", "mesh"), required=True)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--mesh-n", type=int, default=160)
    a = ap.parse_args()
    out = dict(library=os.path.basename(abi.LIB_PATH), method=f"one warm-up render per shape, then {a.runs} timed renders "
               "with XRT_FLAG_TIMING; medians", runs=[])
    if a.scene == "example":
        s = scenes.example(780, 585)
        for spp in (16, 1024):
            for integ in ("whitted", "normal"):
                out["runs"].append(timed(s, 780, 585, spp, a.runs, integrator=integ, max_depth=3))
    else:
        s = mesh_scene(800, 600, a.mesh_n)
        out["scene"] = f"cornell_spheremesh {a.mesh_n} x {a.mesh_n} ({s.desc.n_tris} triangles), glass mesh, point light"
        out["runs"].append(timed(s, 800, 600, 64, a.runs, max_depth=3, whitted_bvh=True))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
