"""tools/wave_timeline.py FILE [--launch N] [--simds 1024] [--cost-map] — the wave timeline of the merged step kernels.

FILE is what an experiment build with -DXRT_PHASE_CLOCK=1 writes for a render when XRT_WAVE_CLOCK_OUT
names it (step_merged.hip, wave_clock_dump): per wave the launch's group argument (all ones: a launch
of every partition), the block, and the constant-rate wall clock and the shader clock at the wave's
entry and exit.  Launches are told apart per group stream: a stream's launches do not overlap, so a
wave that starts after every earlier wave of its stream has ended opens the next launch.

Prints the shader clock (the ratio of the two clocks), the frame's launches per stream, and for one
mid-frame launch (--launch, default the middle one of the first stream) the histogram of wave start
times, the histogram of wave durations and the resident waves over the launch's time; then the
resident waves per SIMD over the middle half of the frame, all streams together — waves' summed
residence inside the window over window x SIMDs, the figure SQ_WAVE_CYCLES x 4 / (time x clock x
SIMDs) estimates from counters.

--cost-map adds, per group stream, where the wave time of its mid-frame launches (the middle half
of them) goes: the mean wave duration per partition — block b of a group's launch serves the
group's partition b % its partition count (step_groups.h), and under the row-major slot map a
partition is a band of image rows — with the spread of those means, the spread of wave durations
inside a launch, and the correlation of a block's mean wave duration between consecutive launches
(Pearson, over the blocks both launches have; the mean over the mid-frame pairs): near 1 when the
same blocks are the slow ones round after round, near 0 when a wave's cost is chance."""
import argparse

import numpy as np

REC = np.dtype([("tag", "<u4"), ("block", "<u4"), ("wall0", "<u8"), ("shader0", "<u8"), ("wall1", "<u8"), ("shader1", "<u8")])


def launches_of(r):
    """indices into r (sorted by entry) of each launch's first wave"""
    first, end = [0], int(r["wall1"][0])
    for i in range(1, len(r)):
        if int(r["wall0"][i]) > end:
            first.append(i)
        end = max(end, int(r["wall1"][i]))
    return first + [len(r)]


def hist(x, lo, hi, bins, unit):
    h, e = np.histogram(x, bins=bins, range=(lo, hi))
    for k in range(bins):
        print(f"  {e[k]:9.1f} .. {e[k + 1]:9.1f} {unit} {h[k]:7d} {'#' * int(60 * h[k] / max(1, h.max()))}")


def resident(t0, t1, lo, hi, bins):
    """mean number of waves resident in each of `bins` equal parts of [lo, hi)"""
    edges = np.linspace(lo, hi, bins + 1)
    out = np.zeros(bins)
    for k in range(bins):
        out[k] = np.clip(np.minimum(t1, edges[k + 1]) - np.maximum(t0, edges[k]), 0, None).sum() / (edges[k + 1] - edges[k])
    return edges, out


def group_part(G, g, lp):
    """step_groups.h step_group_part"""
    return ((lp >> 3) * G + g) * 8 + (lp & 7)


def block_means(w):
    """per block of one launch: mean wave duration in wall ticks (index = block)"""
    b = w["block"].astype(np.int64)
    d = (w["wall1"] - w["wall0"]).astype(np.float64)
    n = np.bincount(b)
    return np.bincount(b, weights=d) / np.maximum(n, 1), n > 0


def cost_map(streams, us):
    for tag in sorted(streams):
        s, L = streams[tag]
        nl = len(L) - 1
        if tag == 0xFFFFFFFF or nl < 8:
            continue
        g, G, parts = tag & 15, (tag >> 4) & 15, tag >> 8
        mid = range(nl // 4, nl - nl // 4)
        print(f"\ncost map, group {g} of {G} ({parts} partitions), launches {mid[0]}..{mid[-1]} of {nl}:")
        psum, pn = np.zeros(parts), np.zeros(parts)
        ratio, cv, corr = [], [], []
        prev = None
        for k in mid:
            w = s[L[k]:L[k + 1]]
            d = (w["wall1"] - w["wall0"]).astype(np.float64) * us
            lp = w["block"].astype(np.int64) % parts
            psum += np.bincount(lp, weights=d, minlength=parts)
            pn += np.bincount(lp, minlength=parts)
            ratio.append(float(np.percentile(d, 99) / np.median(d)))
            cv.append(float(d.std() / d.mean()))
            cur = block_means(w)
            if prev is not None:
                m = min(len(cur[0]), len(prev[0]))
                both = cur[1][:m] & prev[1][:m]
                if both.sum() > 2:
                    corr.append(float(np.corrcoef(cur[0][:m][both], prev[0][:m][both])[0, 1]))
            prev = cur
        pm = psum / np.maximum(pn, 1)
        print(f"  wave durations inside a launch: 99th percentile / median {np.mean(ratio):.2f}, "
              f"standard deviation / mean {np.mean(cv):.3f} (means over the launches)")
        print(f"  block's mean wave duration, launch k against k + 1: correlation {np.mean(corr):.3f} "
              f"(min {np.min(corr):.3f}, max {np.max(corr):.3f}, {len(corr)} pairs)")
        print(f"  mean wave duration per partition: min {pm.min():.0f} us, mean {pm.mean():.0f} us, max {pm.max():.0f} us, "
              f"max / min {pm.max() / pm.min():.2f}")
        print("  partition (group-local -> global): mean wave duration us")
        for lp0 in range(0, parts, 8):
            print("   " + "  ".join(f"{group_part(G, g, lp):3d}:{pm[lp]:5.0f}" for lp in range(lp0, min(lp0 + 8, parts))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("file")
    ap.add_argument("--launch", type=int, default=None)
    ap.add_argument("--simds", type=int, default=1024)
    ap.add_argument("--cost-map", action="store_true")
    a = ap.parse_args()
    head = np.fromfile(a.file, dtype="<u4", count=2)
    n, khz = int(head[0]), int(head[1])
    r = np.fromfile(a.file, dtype=REC, offset=8, count=n)
    r = r[(r["wall1"] > r["wall0"])]
    us = 1e3 / khz   # microseconds per wall tick
    ghz = float((r["shader1"] - r["shader0"]).sum()) / float((r["wall1"] - r["wall0"]).sum()) * khz / 1e6
    print(f"{len(r)} waves of {n} recorded, wall clock {khz / 1e3:.1f} MHz, shader clock {ghz:.3f} GHz")
    t_base = int(r["wall0"].min())
    streams = {}
    for tag in np.unique(r["tag"]):
        s = np.sort(r[r["tag"] == tag], order="wall0")
        streams[int(tag)] = (s, launches_of(s))
        name = "every partition" if tag == 0xFFFFFFFF else f"group {tag & 15} of {(tag >> 4) & 15} ({tag >> 8} partitions)"
        L = streams[int(tag)][1]
        dur = [(int(s["wall1"][L[k]:L[k + 1]].max()) - int(s["wall0"][L[k]])) * us for k in range(len(L) - 1)]
        print(f"stream [{name}]: {len(L) - 1} launches, {len(s)} waves; launch durations us: "
              + " ".join(f"{d:.0f}" for d in dur))
    tag0 = sorted(streams, key=lambda t: -len(streams[t][0]))[0]
    s, L = streams[tag0]
    k = a.launch if a.launch is not None else (len(L) - 1) // 2
    w = s[L[k]:L[k + 1]]
    lo, hi = int(w["wall0"].min()), int(w["wall1"].max())
    t0, t1 = (w["wall0"].astype(np.int64) - lo) * us, (w["wall1"].astype(np.int64) - lo) * us
    span = (hi - lo) * us
    print(f"\nlaunch {k} of that stream: {len(w)} waves in {len(np.unique(w['block']))} blocks, {span:.0f} us, "
          f"starting {(lo - t_base) * us:.0f} us into the frame")
    print("wave start times:")
    hist(t0, 0.0, span, 10, "us")
    print("wave durations:")
    hist(t1 - t0, 0.0, span, 10, "us")
    late = t0 > 0.25 * span
    print(f"waves starting in the first quarter: {int((~late).sum())}, mean duration {float((t1 - t0)[~late].mean()):.0f} us; "
          f"later: {int(late.sum())}" + (f", mean duration {float((t1 - t0)[late].mean()):.0f} us" if late.any() else ""))
    print(f"resident waves of this launch over its time (per SIMD of {a.simds}):")
    e, res = resident(t0, t1, 0.0, span, 10)
    for q in range(10):
        print(f"  {e[q]:9.1f} .. {e[q + 1]:9.1f} us {res[q]:8.0f} {res[q] / a.simds:5.2f}")
    print(f"  whole launch: {float((t1 - t0).sum()) / span / a.simds:.2f} per SIMD")
    # the middle half of the frame, every stream
    f0, f1 = int(r["wall0"].min()), int(r["wall1"].max())
    m0, m1 = f0 + (f1 - f0) // 4, f1 - (f1 - f0) // 4
    inside = np.clip(np.minimum(r["wall1"].astype(np.int64), m1) - np.maximum(r["wall0"].astype(np.int64), m0), 0, None).sum()
    print(f"\nframe: {(f1 - f0) * us / 1e3:.2f} ms of step launches; resident waves per SIMD over its middle half: "
          f"{inside / (m1 - m0) / a.simds:.2f}")
    whole = float((r["wall1"] - r["wall0"]).sum()) / (f1 - f0) / a.simds
    print(f"over the whole of it: {whole:.2f}")
    if a.cost_map:
        cost_map(streams, us)


if __name__ == "__main__":
    main()
