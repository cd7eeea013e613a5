#!/usr/bin/env python3
"""tools/denoise_bench.py — time the edge-avoiding a-trous filter (xrt_denoise_device, all four
guide planes, device tensors in and out) on one GPU, and print one JSON object: what
profiles/denoise_example.json records.

The frame is the scene of examples/denoise.cpp (the example's plane and sphere under a QuadLight)
rendered on the GPU with GIIntegrator(3) at 4 spp, with its guide buffers, at 800 x 600 and
1920 x 1080.  Per size and iteration count: one warm-up call of each path, then --runs timed
calls, the default path and XRT_DENOISE_NO_TILE alternating within the process, with
XRT_DENOISE_TIMING; kernel time is the HIP events round every launch (the prepass included), wall
time the library's clock round the call (it ends in a stream synchronise); medians.  The headline
is 5 iterations; the sweep over 1 .. 5 iterations gives each step's cost by difference, which is
what fixes XRT_DENOISE_TILED_ITERATIONS.

Bytes are computed from shapes: as executed, an iteration reads 25 taps x 48 B and writes 16 B per
pixel; the compulsory floor is 48 B read and 16 B written per pixel and iteration."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch   # noqa: E402

from xraytracer_amd import abi, scenes   # noqa: E402
from xraytracer_amd.renderer import HipRenderer   # noqa: E402

SIZES = ((800, 600), (1920, 1080))
SIGMAS = dict(sigma_color=2.0, sigma_normal=0.5, sigma_depth=1.0, sigma_albedo=0.2)


def scene(w, h):
    s = scenes.SceneBundle()
    s.add_mesh("plane", scenes.EXAMPLE_PLANE, (1.0, 1.0, 1.0))
    s.add_sphere("sphere_diffuse", (0.0, 0.0, 0.0), 1.0, (0.58, 0.58, 0.58))
    s.add_quad_light("QuadLight", (1.0, 4.0, -1.0), (1.0, 4.0, 1.0), (-1.0, 4.0, -1.0), (25.0, 25.0, 25.0))
    s.flatten()
    s.camera = scenes.pinhole((1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 8, 1), 60.0, w, h)
    s.integrator, s.max_depth = "gi", 3
    return s


def traffic(w, h, iterations):
    px = w * h
    return dict(executed_bytes=px * iterations * (25 * 48 + 16), floor_bytes=px * iterations * (48 + 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--spp", type=int, default=4)
    ap.add_argument("--iterations", type=int, default=5)
    a = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    out = dict(library=os.path.basename(abi.LIB_PATH), abi_version=abi.XRT_ABI_VERSION,
               tiled_iterations_constant=abi.XRT_DENOISE_TILED_ITERATIONS, settings=SIGMAS,
               method=f"per size and iteration count one warm-up call of each path, then {a.runs} timed calls of each, "
                      "alternating, with XRT_DENOISE_TIMING; medians", runs=[])
    r = HipRenderer(a.spp)
    try:
        for w, h in SIZES:
            s = scene(w, h)
            frame = torch.zeros((h, w, 3), dtype=torch.float32, device="cuda:0")
            result = torch.zeros_like(frame)
            planes = {k: torch.zeros((h, w, 3) if k in ("albedo", "normal") else (h, w),
                                     dtype=torch.int32 if k == "object" else torch.float32, device="cuda:0")
                      for k in abi.DENOISE_PLANES}
            render = r.render_device(s, w, h, frame.data_ptr(), after_stream=stream, timing=True)
            guides = r.render_aov_device(s, w, h, {k: v.data_ptr() for k, v in planes.items()}, after_stream=stream,
                                         timing=True)
            ptrs = {k: v.data_ptr() for k, v in planes.items()}

            def call(tile, iterations):
                return r.denoise_device(frame.data_ptr(), ptrs, result.data_ptr(), w, h, after_stream=stream,
                                        iterations=iterations, tile=tile, timing=True, **SIGMAS)

            for iterations in sorted(set(range(1, a.iterations + 1))):
                paths = (("default", True), ("no_tile", False))
                rec = {name: ([], []) for name, _ in paths}
                last = {}
                for name, tile in paths:
                    call(tile, iterations)
                for _ in range(a.runs):
                    for name, tile in paths:
                        st = call(tile, iterations)
                        rec[name][0].append(st.wall_ms)
                        rec[name][1].append(st.kernel_ms)
                        last[name] = st
                t = traffic(w, h, iterations)
                for name, _ in paths:
                    km = statistics.median(rec[name][1])
                    out["runs"].append(dict(
                        what=name, width=w, height=h, iterations=iterations, launches=int(last[name].launches),
                        tiled_iterations=int(last[name].tiled_iterations), direct_iterations=int(last[name].direct_iterations),
                        wall_ms=rec[name][0], wall_ms_median=statistics.median(rec[name][0]), kernel_ms=rec[name][1],
                        kernel_ms_median=km, executed_tb_per_s=t["executed_bytes"] / km / 1e9,
                        floor_tb_per_s=t["floor_bytes"] / km / 1e9, **t))
            out["runs"].append(dict(what="frame", width=w, height=h, spp=a.spp, render_wall_ms=render.wall_ms,
                                    guides_wall_ms=guides.wall_ms))
    finally:
        r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
