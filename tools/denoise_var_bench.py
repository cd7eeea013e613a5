#!/usr/bin/env python3
"""tools/denoise_var_bench.py — time the variance-guided a-trous filter (xrt_denoise_var_device, all
four guide planes, device tensors in and out) on one GPU beside xrt_denoise_device as the yardstick,
and print one JSON object: what profiles/denoise_var_example.json records.

The frame is tools/denoise_bench.py's (the scene of examples/denoise.cpp rendered on the GPU with
GIIntegrator(3) at 4 spp, with its guide buffers) at 800 x 600 and 1920 x 1080.  Per size and
iteration count: one warm-up call of each path, then --runs timed calls of each, the paths
alternating within the process, with XRT_DENOISE_TIMING; kernel time is the HIP events round every
launch (the prepass and the estimate included), wall time the library's clock round the call;
medians.  The paths:
  var_default   xrt_denoise_var, variance estimated (radius 3), the default kernels
  var_no_tile   the same under XRT_DENOISE_NO_TILE
  var_supplied  the default kernels with a caller's variance plane (the variance one pass of the
                filter leaves on the same frame), so var_default - var_supplied is the estimate
                launch on its own
  plain_default / plain_no_tile   xrt_denoise at the same size and iteration count
The sweep over 1 .. 5 iterations gives each step's cost by difference, tiled (var_default) against
direct (var_no_tile): what fixes XRT_DENOISE_VAR_TILED_ITERATIONS.

Bytes are computed from shapes: as executed, an iteration reads 25 taps x 48 B and 9 variance words
and writes 16 B per pixel; the compulsory floor is 48 B read and 16 B written per pixel and iteration."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch   # noqa: E402

from denoise_bench import SIZES, scene   # noqa: E402
from xraytracer_amd import abi   # noqa: E402
from xraytracer_amd.renderer import HipRenderer   # noqa: E402

GUIDE_SIGMAS = dict(sigma_normal=0.5, sigma_depth=1.0, sigma_albedo=0.2)
VAR = dict(sigma_luminance=4.0, variance_radius=3, **GUIDE_SIGMAS)
PLAIN = dict(sigma_color=2.0, **GUIDE_SIGMAS)


def traffic(w, h, iterations, var):
    px = w * h
    return dict(executed_bytes=px * iterations * (25 * 48 + (9 * 4 if var else 0) + 16), floor_bytes=px * iterations * (48 + 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=5)
    a = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    out = dict(library=os.path.basename(abi.LIB_PATH), abi_version=abi.XRT_ABI_VERSION,
               var_tiled_iterations_constant=abi.XRT_DENOISE_VAR_TILED_ITERATIONS,
               tiled_iterations_constant=abi.XRT_DENOISE_TILED_ITERATIONS, var_settings=VAR, plain_settings=PLAIN,
               method=f"per size and iteration count one warm-up call of each path, then {a.runs} timed calls of each, "
                      "alternating, with XRT_DENOISE_TIMING; medians", runs=[])
    r = HipRenderer(a.spp)
    try:
        for w, h in SIZES:
            s = scene(w, h)
            frame = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
            result = torch.zeros_like(frame)
            variance = torch.zeros((h, w), dtype=torch.float32, device="cuda:0")
            result_var = torch.zeros_like(variance)
            planes = {k: torch.zeros((h, w, 3) if k in ("albedo", "normal") else (h, w),
                                     dtype=torch.int32 if k == "object" else torch.float32, device="cuda:0")
                      for k in abi.DENOISE_PLANES}
            ptrs = {k: v.data_ptr() for k, v in planes.items()}
            r.render_device(s, w, h, frame.data_ptr(), after_stream=stream)
            r.render_aov_device(s, w, h, ptrs, after_stream=stream)
            # a realistic caller's plane: the variance one pass leaves
            r.denoise_var_device(frame.data_ptr(), ptrs, result.data_ptr(), w, h, out_variance_ptr=variance.data_ptr(),
                                 after_stream=stream, iterations=1, **VAR)

            def var_call(tile, supplied, iterations):
                return r.denoise_var_device(frame.data_ptr(), ptrs, result.data_ptr(), w, h,
                                            variance_ptr=variance.data_ptr() if supplied else 0,
                                            out_variance_ptr=result_var.data_ptr(), after_stream=stream, iterations=iterations,
                                            tile=tile, timing=True, **VAR)

            def plain_call(tile, iterations):
                return r.denoise_device(frame.data_ptr(), ptrs, result.data_ptr(), w, h, after_stream=stream,
                                        iterations=iterations, tile=tile, timing=True, **PLAIN)

            paths = (("var_default", lambda n: var_call(True, False, n)), ("var_no_tile", lambda n: var_call(False, False, n)),
                     ("var_supplied", lambda n: var_call(True, True, n)), ("plain_default", lambda n: plain_call(True, n)),
                     ("plain_no_tile", lambda n: plain_call(False, n)))
            for iterations in range(1, a.iterations + 1):
                rec = {name: ([], []) for name, _ in paths}
                last = {}
                for name, fn in paths:
                    fn(iterations)
                for _ in range(a.runs):
                    for name, fn in paths:
                        st = fn(iterations)
                        rec[name][0].append(st.wall_ms)
                        rec[name][1].append(st.kernel_ms)
                        last[name] = st
                for name, _ in paths:
                    km = statistics.median(rec[name][1])
                    t = traffic(w, h, iterations, name.startswith("var"))
                    out["runs"].append(dict(
                        what=name, width=w, height=h, iterations=iterations, launches=int(last[name].launches),
                        tiled_iterations=int(last[name].tiled_iterations), direct_iterations=int(last[name].direct_iterations),
                        wall_ms=rec[name][0], wall_ms_median=statistics.median(rec[name][0]), kernel_ms=rec[name][1],
                        kernel_ms_median=km, executed_tb_per_s=t["executed_bytes"] / km / 1e9,
                        floor_tb_per_s=t["floor_bytes"] / km / 1e9, **t))
    finally:
        r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
