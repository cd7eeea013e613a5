"""tools/wave_timeline.py FILE [--launch N] [--simds 1024] [--cost-map] [--chunks [--live64 N]] — the wave timeline of the merged step kernels.

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
same blocks are the slow ones round after round, near 0 when a wave's cost is chance.

--chunks reports the chunk phase (k_step_merged_chunks, whose waves carry the tag 0xFFFFFFFE) from the
pass-end records the file holds behind the waves' (step_sources.h, PassClockRec: per wave and barrier
of a pass end the wall clock before and after it, with the wave's survivors of the pass):
  (a) the share of the phase's wave time spent between `before` and `after` of those barriers;
  (b) per launch, the time from the median block's end to the launch's end (the drain) and the gap to
      the next launch's first wave; for the middle launch, the mean block end per quarter of the block
      index, which is the order of dispatch;
  (c) the duration of a wave's pass — from its entry or the end of its previous pass to its arrival at
      the pass end — first passes (which hold the LDS scene copy) apart from the others;
  (d) the live slots each launch leaves (the survivors of every wave's last pass: exact where a block
      owns one chunk), the launches that started below --live64
      (kMergedLive64) and what they cost.
(a) + (b) + (d) is what a schedule without pass barriers, drains or overrun could gain at most."""
import argparse

import numpy as np

REC = np.dtype([("tag", "<u4"), ("block", "<u4"), ("wall0", "<u8"), ("shader0", "<u8"), ("wall1", "<u8"), ("shader1", "<u8")])
PASS = np.dtype([("block", "<u4"), ("wave_kind", "<u4"), ("n", "<u4"), ("pad", "<u4"), ("before", "<u8"), ("after", "<u8")])
CHUNK_TAG = 0xFFFFFFFE


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
        if tag in (0xFFFFFFFF, CHUNK_TAG) or nl < 8:
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


def chunk_report(s, L, pr, us, live64, frame_us):
    """s: the chunk kernel's waves sorted by entry, L: its launches (launches_of), pr: the pass-end records"""
    nl = len(L) - 1
    pr = pr[pr["after"] >= pr["before"]]
    pr = np.sort(pr, order="before")
    starts = np.array([int(s["wall0"][L[k]]) for k in range(nl)], dtype=np.int64)
    ends = np.array([int(s["wall1"][L[k]:L[k + 1]].max()) for k in range(nl)], dtype=np.int64)
    phase_us = (ends[-1] - starts[0]) * us
    wave_time = float((s["wall1"] - s["wall0"]).sum()) * us
    print(f"\nchunk phase: {nl} launches, {len(s)} waves, {len(pr)} pass-end records, {phase_us / 1e3:.2f} ms "
          f"({100 * phase_us / frame_us:.1f} % of the frame's step time), wave time {wave_time / 1e3:.0f} ms summed")
    # (a) barrier waits
    wait = (pr["after"] - pr["before"]).astype(np.float64) * us
    kind = pr["wave_kind"] >> 8
    print(f"(a) waiting at pass-end barriers: {100 * wait.sum() / wave_time:.2f} % of the phase's wave time "
          + ", ".join(f"kind {k}: {100 * wait[kind == k].sum() / wave_time:.2f} % (mean {wait[kind == k].mean():.1f} us, "
                      f"99th percentile {np.percentile(wait[kind == k], 99):.1f} us, {int((kind == k).sum())} waits)"
                      for k in np.unique(kind)))
    a_ms = wait.sum() / wave_time * phase_us / 1e3
    print(f"    as time of the phase at that share: {a_ms:.3f} ms")
    # (b) drain and gap per launch
    drain, gap = [], []
    for k in range(nl):
        w = s[L[k]:L[k + 1]]
        b = w["block"].astype(np.int64)
        bend = np.zeros(b.max() + 1, dtype=np.int64)
        np.maximum.at(bend, b, w["wall1"].astype(np.int64))
        bend = bend[np.bincount(b) > 0]
        drain.append((int(ends[k]) - float(np.median(bend))) * us)
        if k + 1 < nl:
            gap.append((int(starts[k + 1]) - int(ends[k])) * us)
    print("(b) launch us / median block's end to launch end us / gap to the next launch's first wave us:")
    for k in range(nl):
        print(f"    launch {k:2d}: {(ends[k] - starts[k]) * us:8.0f} {drain[k]:7.1f} " + (f"{gap[k]:7.1f}" if k < len(gap) else "      -"))
    b_ms = (sum(drain) + sum(gap)) / 1e3
    print(f"    drains {sum(drain) / 1e3:.3f} ms + gaps {sum(gap) / 1e3:.3f} ms = {b_ms:.3f} ms")
    # who drains: a block's end against its index (the order of dispatch), the middle launch
    k = nl // 2
    w = s[L[k]:L[k + 1]]
    b = w["block"].astype(np.int64)
    bend = np.zeros(b.max() + 1)
    np.maximum.at(bend, b, (w["wall1"].astype(np.int64) - int(starts[k])) * us)
    nb = len(bend)
    print(f"    launch {k}: mean block end us by quarter of the block index (dispatch order): "
          + " ".join(f"{bend[q * nb // 4:(q + 1) * nb // 4].mean():.0f}" for q in range(4))
          + f"; all blocks had started after {(int(w['wall0'].max()) - int(starts[k])) * us:.0f} us")
    # (c) a wave's pass: from its entry or its previous pass end to its arrival at the pass end
    key_w = s["block"].astype(np.int64)
    first_d, later_d, live_after = [], [], []
    for k in range(nl):
        w = s[L[k]:L[k + 1]]
        q = pr[(pr["before"] >= starts[k]) & (pr["before"] <= ends[k])]
        wid = q["block"].astype(np.int64) * 16 + (q["wave_kind"] & 255).astype(np.int64)
        last_n = {}
        prev_end = {}
        arr = {}
        for i in np.argsort(q["before"], kind="stable"):
            key, kd = int(wid[i]), int(q["wave_kind"][i]) >> 8
            if kd == 0 or key not in arr:
                arr.setdefault(key, []).append([int(q["before"][i]), int(q["after"][i])])
                if kd == 0:
                    last_n[key] = int(q["n"][i])
            else:
                arr[key][-1][1] = int(q["after"][i])
        # waves enter in any order within a block: pair a block's waves with its entry clocks by order
        ent = {}
        for b, t in zip(w["block"].astype(np.int64), w["wall0"].astype(np.int64)):
            ent.setdefault(int(b), []).append(int(t))
        for key, ps in arr.items():
            t_in = min(ent.get(key // 16, [ps[0][0]]))
            first_d.append((ps[0][0] - t_in) * us)
            for j in range(1, len(ps)):
                later_d.append((ps[j][0] - ps[j - 1][1]) * us)
        live_after.append(sum(last_n.values()))
    first_d, later_d = np.array(first_d), np.array(later_d)
    print(f"(c) a wave's pass (64 visits at most) at the phase's residency: first passes of a launch, from the block's "
          f"first entry (LDS scene copy included) median {np.median(first_d):.0f} us, mean {first_d.mean():.0f}; later passes "
          f"median {np.median(later_d):.0f} us, mean {later_d.mean():.0f}, standard deviation / mean "
          f"{later_d.std() / later_d.mean():.3f}, 99th percentile / median {np.percentile(later_d, 99) / np.median(later_d):.2f}")
    # (d) launches past the threshold
    print(f"(d) live slots left by each launch: " + " ".join(str(v) for v in live_after))
    past = [k for k in range(1, nl) if live_after[k - 1] < live64]
    d_ms = sum((ends[k] - starts[k]) * us for k in past) / 1e3
    print(f"    launches that started below {live64} live slots: {len(past)}" + (f" (launches {past})" if past else "")
          + f", {d_ms:.3f} ms")
    # the first launch to cross: the part of it after the crossing is not told apart here
    tot = a_ms + b_ms + d_ms
    print(f"(a) + (b) + (d) = {a_ms:.3f} + {b_ms:.3f} + {d_ms:.3f} = {tot:.3f} ms, {100 * tot * 1e3 / frame_us:.2f} % of the "
          f"frame's {frame_us / 1e3:.2f} ms of step launches")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("file")
    ap.add_argument("--launch", type=int, default=None)
    ap.add_argument("--simds", type=int, default=1024)
    ap.add_argument("--cost-map", action="store_true")
    ap.add_argument("--chunks", action="store_true")
    ap.add_argument("--live64", type=int, default=160000, help="kMergedLive64 (wavefront.h)")
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
        name = "every partition" if tag == 0xFFFFFFFF else "chunks" if tag == CHUNK_TAG else f"group {tag & 15} of {(tag >> 4) & 15} ({tag >> 8} partitions)"
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
    if a.chunks:
        off = 8 + n * REC.itemsize
        m = int(np.fromfile(a.file, dtype="<u4", count=1, offset=off)[0])
        pr = np.fromfile(a.file, dtype=PASS, offset=off + 4, count=m)
        if CHUNK_TAG not in streams:
            print("\nno chunk launches in this file")
        else:
            chunk_report(*streams[CHUNK_TAG], pr, us, a.live64, (f1 - f0) * us)


if __name__ == "__main__":
    main()
