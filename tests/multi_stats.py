"""What a multi-device context reports in xrt_stats, from its devices' own stats: every
counter is the sum over the devices, except `iterations` (the longest device's) and the
schedule's description (device 0's).  The fields are read from abi.XrtStats, so a field added
to xrt_stats is expected to be summed until it is listed here."""
from xraytracer_amd import abi

TIMINGS = ("wall_ms", "kernel_ms")
FROM_FIRST = ("schedule", "partitions", "visits_per_launch", "slots_per_wave", "group_lanes")
# how many launches a looping schedule (GI, VPT) takes follows the timing of its live-count
# polls, so two renders of the same shard need not agree on these
LOOP_LENGTH = ("iterations", "launches", "layout_launches", "spec_launches")


def counters(st, skip=()):
    """xrt_stats as {field: int or tuple of ints}, without the timings"""
    out = {}
    for name, _ in abi.XrtStats._fields_:
        if name in TIMINGS or name in skip:
            continue
        v = getattr(st, name)
        out[name] = tuple(int(x) for x in v) if hasattr(v, "__len__") else int(v)
    return out


def combined(parts):
    """the multi-device stats for the per-device counters() `parts`, device 0 first"""
    out = {}
    for k, v in parts[0].items():
        vals = [p[k] for p in parts]
        if k in FROM_FIRST:
            out[k] = v
        elif k == "iterations":
            out[k] = max(vals)
        elif isinstance(v, tuple):
            out[k] = tuple(sum(col) for col in zip(*vals))
        else:
            out[k] = sum(vals)
    return out
