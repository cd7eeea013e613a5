#!/usr/bin/env python3
"""tools/progressive_bench.py — time a progressive session (xrt_progressive_*) beside the one-shot render
it continues, on one GPU, and print one JSON object: what profiles/progressive_example.json records.

Workload: C2's Cornell box at 800 x 600 under GIIntegrator(3), 1,024 spp in all.  Compared:
  render_nospec       xrt_render_device at 1,024 spp with XRT_FLAG_NO_SPEC: one shot, no speculative starts
  session_1x1024      begin, one add of 1,024 spp, frame_device
  session_16x64       begin, 16 adds of 64 spp, frame_device
  session_64x16       begin, 64 adds of 16 spp, frame_device
  frame_device        one xrt_progressive_frame_device of the finished 64 x 16 session (wall clock round the call)
  resume_kernel       k_resume's HIP-event time per add, from a 16 x 64 session with XRT_FLAG_TIMING and
                      XRT_FLAG_NO_CHUNKS (nothing else of such an add counts under XRT_K_SEED)
A session's time is the wall clock round begin .. frame_device.  One warm-up of each, then --runs timed
runs of each, alternating; medians.  Every session's frame is compared with the one-shot frame, bit for
bit, before its time is recorded."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch   # noqa: E402

from xraytracer_amd import abi, scenes   # noqa: E402
from xraytracer_amd.renderer import HipRenderer   # noqa: E402

W, H, TOTAL = 800, 600, 1024
SPLITS = (("session_1x1024", 1, 1024), ("session_16x64", 16, 64), ("session_64x16", 64, 16))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--total", type=int, default=TOTAL, help="samples per pixel in all (a multiple of 64)")
    a = ap.parse_args()
    scale = a.total / TOTAL
    s = scenes.build("C2")
    stream = torch.cuda.current_stream().cuda_stream
    one = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    frame = torch.zeros((H, W, 3), dtype=torch.float32, device="cuda:0")
    r = HipRenderer(a.total)
    kw = dict(integrator="gi", max_depth=3)
    frame_ms, resume_ms, resume_twists = [], [], []

    def render():
        t = time.perf_counter()
        st = r.render_device(s, W, H, one.data_ptr(), after_stream=stream, spec=False, **kw)
        return 1e3 * (time.perf_counter() - t), st

    def session(adds, spp, timing=False, **more):
        t = time.perf_counter()
        with r.progressive(s, W, H, timing=timing, **kw, **more) as ps:
            per_add = []
            for _ in range(adds):
                st = ps.add(spp)
                per_add.append((st.kernel_ms[abi.XRT_K_SEED], ps.state.resume_twists if timing else 0))
            t_frame = time.perf_counter()
            ps.frame_device(frame.data_ptr(), after_stream=stream)
            t_end = time.perf_counter()
        torch.cuda.synchronize()
        assert torch.equal(frame.view(torch.int32), one.view(torch.int32)), "the session's frame is not the one-shot frame"
        return 1e3 * (t_end - t), st, 1e3 * (t_end - t_frame), per_add

    try:
        calls = [("render_nospec", render)] + [(n, (lambda k=k, q=q: session(k, int(q * scale)))) for n, k, q in SPLITS]
        rec = {n: [] for n, _ in calls}
        last = {}
        for _, fn in calls:   # warm-up: code objects, buffers, the upload; the one-shot frame first
            fn()
        for _ in range(a.runs):
            for n, fn in calls:
                got = fn()
                rec[n].append(got[0])
                last[n] = got[1]
                if n == "session_64x16":
                    frame_ms.append(got[2])
        _, _, _, per_add = session(16, int(64 * scale), timing=True, chunks=False)
        resume_ms = [q[0] for q in per_add]
        resume_twists = [int(q[1]) for q in per_add]
    finally:
        r.close()
    out = dict(library=os.path.basename(abi.LIB_PATH), abi_version=abi.XRT_ABI_VERSION, workload="c2_cornell", width=W, height=H,
               spp_total=a.total,
               method=f"one warm-up of each, then {a.runs} timed runs of each, alternating; wall clock round the call "
                      "(a session: begin .. frame_device); medians; every session frame checked bit for bit against the one-shot frame",
               runs=[])
    for n, _ in calls:
        st = last[n]
        out["runs"].append(dict(what=n, schedule=int(st.schedule), samples=int(st.samples), segments=int(st.segments),
                                wall_ms=rec[n], wall_ms_median=statistics.median(rec[n]), wall_ms_range=[min(rec[n]), max(rec[n])]))
    base = statistics.median(rec["render_nospec"])
    out["runs"].append(dict(what="ratios_of_wall_ms_medians",
                            **{f"{n}_over_render_nospec": statistics.median(rec[n]) / base for n, _, _ in SPLITS}))
    out["runs"].append(dict(what="frame_device", wall_ms=frame_ms, wall_ms_median=statistics.median(frame_ms)))
    out["runs"].append(dict(what="resume_kernel", adds=16, spp_per_add=int(64 * scale), kernel_ms_per_add=resume_ms,
                            kernel_ms_median=statistics.median(resume_ms), kernel_ms_first_add=resume_ms[0],
                            resume_twists_per_add=resume_twists, path_slots=W * H))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
