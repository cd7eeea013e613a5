#!/usr/bin/env python3
"""tools/aov_bench.py — time the guide-buffer pass (xrt_render_aov_device, all five planes into
device memory) beside NormalIntegrator renders on k_pixel, on one GPU, and print one JSON object:
what profiles/aov_example.json records.

The scene is scenes.example at 780 x 585, at 16 and 1024 spp.  Normal on the pixel schedule is
one Scene::intersect per sample over the same camera rays, the structural floor of the guide
pass for this scene.  Per spp: one warm-up call of each, then --runs timed calls of each,
alternating, with XRT_FLAG_TIMING; wall time is the library's clock around the call (it ends in
a stream synchronise), kernel time the HIP events around the one XRT_K_STEP launch; medians.

--normal-only times just the Normal renders and touches nothing the guide pass added, so the
same file can be run against an older build of the library for the baseline."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch   # noqa: E402

from xraytracer_amd import abi, scenes   # noqa: E402
from xraytracer_amd.renderer import HipRenderer   # noqa: E402

W, H = 780, 585


def summary(name, st, wall, step, spp):
    wm, sm = statistics.median(wall), statistics.median(step)
    return dict(what=name, width=W, height=H, spp=spp, schedule=int(st.schedule), samples=int(st.samples),
                segments=int(st.segments), wall_ms=wall, wall_ms_median=wm, kernel_ms_step=step, kernel_ms_step_median=sm,
                msamples_per_s_kernel=st.samples / sm / 1e3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--normal-only", action="store_true")
    a = ap.parse_args()
    s = scenes.example(W, H)
    stream = torch.cuda.current_stream().cuda_stream
    frame = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    planes = None
    if not a.normal_only:
        planes = {k: torch.zeros((H, W, 3) if k in ("albedo", "normal") else (H, W),
                                 dtype=torch.int32 if k == "object" else torch.float32, device="cuda:0")
                  for k in abi.AOV_PLANES}
    out = dict(library=os.path.basename(abi.LIB_PATH), abi_version=abi.XRT_ABI_VERSION,
               method=f"per spp one warm-up call of each, then {a.runs} timed calls of each, alternating, with "
                      "XRT_FLAG_TIMING; medians", runs=[])
    for spp in (16, 1024):
        r = HipRenderer(spp)
        try:
            def normal():
                return r.render_device(s, W, H, frame.data_ptr(), after_stream=stream, integrator="normal", timing=True)

            def guides():
                return r.render_aov_device(s, W, H, {k: v.data_ptr() for k, v in planes.items()}, after_stream=stream,
                                           timing=True)

            calls = [("normal_k_pixel", normal)] + ([] if a.normal_only else [("aov_all_planes", guides)])
            rec = {name: ([], []) for name, _ in calls}
            last = {}
            for name, fn in calls:   # warm-up: code objects, buffers, the upload
                fn()
            for _ in range(a.runs):
                for name, fn in calls:
                    st = fn()
                    rec[name][0].append(st.wall_ms)
                    rec[name][1].append(st.kernel_ms[abi.XRT_K_STEP])
                    last[name] = st
            for name, _ in calls:
                out["runs"].append(summary(name, last[name], rec[name][0], rec[name][1], spp))
            if not a.normal_only:
                n, g = (statistics.median(rec[k][1]) for k in ("normal_k_pixel", "aov_all_planes"))
                out["runs"].append(dict(what="aov_over_normal_kernel_ms_step", spp=spp, ratio=g / n))
        finally:
            r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
