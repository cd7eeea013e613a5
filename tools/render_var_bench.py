#!/usr/bin/env python3
"""tools/render_var_bench.py — time the variance render (xrt_render_var_device) beside the renders
it is made of, on one GPU, and print one JSON object: what profiles/render_var_example.json records.

Workloads: scenes.example at 780 x 585 and C2's Cornell box at 800 x 600, under GIIntegrator(3), at
16 and 64 spp.  On each, five calls are compared:
  render_var            xrt_render_var_device: the wavefront schedule with the moments build of k_shade
                        and k_finish_var
  render_wavefront      xrt_render_device with XRT_FLAG_WAVEFRONT: the same kernels without moments
  render_default        xrt_render_device at the schedule the library chooses
  render_var_fused      xrt_render_var_device with XRT_FLAG_VAR_FUSED: the fused or merged schedule with
                        the moments builds of k_step / k_step_merged
  render_nospec_nopixel xrt_render_device with XRT_FLAG_NO_SPEC | XRT_FLAG_NO_PIXEL: the same kernels
                        without moments
render_var / render_wavefront and render_var_fused / render_nospec_nopixel are what the moments cost in
either schedule, render_wavefront / render_default what forcing the wavefront schedule costs,
render_var / render_var_fused what the flag buys.  Per workload: one warm-up call of each, then --runs timed
calls of each, alternating, with XRT_FLAG_TIMING; kernel time is the sum of the HIP-event times
round every launch of the call, wall time the library's clock round the call; medians."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch   # noqa: E402

from xraytracer_amd import abi, scenes   # noqa: E402
from xraytracer_amd.renderer import HipRenderer   # noqa: E402

WORKLOADS = (("example", lambda: scenes.example(780, 585), 780, 585), ("c2_cornell", lambda: scenes.build("C2"), 800, 600))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    a = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    out = dict(library=os.path.basename(abi.LIB_PATH), abi_version=abi.XRT_ABI_VERSION,
               method=f"per workload one warm-up call of each, then {a.runs} timed calls of each, alternating, with "
                      "XRT_FLAG_TIMING; kernel_ms is the sum over the call's launches; medians", runs=[])
    for wname, make, w, h in WORKLOADS:
        s = make()
        frame = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
        var = torch.zeros((h, w), dtype=torch.float32, device="cuda:0")
        for spp in (16, 64):
            r = HipRenderer(spp)
            try:
                kw = dict(after_stream=stream, integrator="gi", max_depth=3, timing=True)
                calls = [("render_var", lambda: r.render_var_device(s, w, h, frame.data_ptr(), var.data_ptr(), **kw)),
                         ("render_wavefront", lambda: r.render_device(s, w, h, frame.data_ptr(), schedule="wavefront", **kw)),
                         ("render_default", lambda: r.render_device(s, w, h, frame.data_ptr(), **kw)),
                         ("render_var_fused", lambda: r.render_var_device(s, w, h, frame.data_ptr(), var.data_ptr(),
                                                                          fused_var=True, **kw)),
                         ("render_nospec_nopixel", lambda: r.render_device(s, w, h, frame.data_ptr(), spec=False,
                                                                           schedule="step", **kw))]
                rec = {name: ([], []) for name, _ in calls}
                last = {}
                for _, fn in calls:   # warm-up: code objects, buffers, the upload
                    fn()
                for _ in range(a.runs):
                    for name, fn in calls:
                        st = fn()
                        rec[name][0].append(st.wall_ms)
                        rec[name][1].append(sum(st.kernel_ms))
                        last[name] = st
                med, wall = {}, {}
                for name, _ in calls:
                    st = last[name]
                    med[name] = statistics.median(rec[name][1])
                    wall[name] = statistics.median(rec[name][0])
                    out["runs"].append(dict(what=name, workload=wname, width=w, height=h, spp=spp, schedule=int(st.schedule),
                                            samples=int(st.samples), segments=int(st.segments), wall_ms=rec[name][0],
                                            wall_ms_median=statistics.median(rec[name][0]), kernel_ms=rec[name][1],
                                            kernel_ms_median=med[name], kernel_ms_range=[min(rec[name][1]), max(rec[name][1])],
                                            wall_ms_range=[min(rec[name][0]), max(rec[name][0])],
                                            kernel_ms_by_kernel={n: st.kernel_ms[i] for i, n in enumerate(abi.KERNEL_NAMES)}))
                out["runs"].append(dict(what="ratios_of_kernel_ms_medians", workload=wname, spp=spp,
                                        moments_cost_var_over_wavefront=med["render_var"] / med["render_wavefront"],
                                        schedule_cost_wavefront_over_default=med["render_wavefront"] / med["render_default"],
                                        moments_cost_var_fused_over_nospec_nopixel=med["render_var_fused"] / med["render_nospec_nopixel"],
                                        gain_var_over_var_fused=med["render_var"] / med["render_var_fused"]))
                out["runs"].append(dict(what="ratios_of_wall_ms_medians", workload=wname, spp=spp,
                                        moments_cost_var_fused_over_nospec_nopixel=wall["render_var_fused"] / wall["render_nospec_nopixel"],
                                        gain_var_over_var_fused=wall["render_var"] / wall["render_var_fused"]))
            finally:
                r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
