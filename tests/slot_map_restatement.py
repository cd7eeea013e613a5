"""The slot -> pixel map of xraytracer_amd/csrc/slot_map.h and host/slot_map.cpp, restated in Python —
a helper, not a test module.  tests/test_slot_map.py holds it against the C++ (CPU), and
tests/test_gpu_interleave.py holds the device's map (xrt_test_slot_map) against it."""
import math

import numpy as np


def multiplier(n: int) -> int:
    """the smallest A >= round(0.3819660113 n) coprime to n; 0 (the row-major map) for n <= 1"""
    if n <= 1:
        return 0
    a = max(1, int(0.3819660113 * n + 0.5))
    while math.gcd(a, n) != 1:
        a += 1
    return a


def pixels(width: int, height: int, shard_index: int = 0, shard_count: int = 1, interleave: bool = True) -> np.ndarray:
    """per slot of the shard the pixel index col + width * row"""
    rows = len(range(shard_index, height, shard_count))
    n = width * rows
    s = np.arange(n, dtype=np.uint64)
    mul = multiplier(n) if interleave else 0
    q = (s * np.uint64(mul)) % np.uint64(n) if mul else s
    col, row = q % np.uint64(width), np.uint64(shard_index) + np.uint64(shard_count) * (q // np.uint64(width))
    return (col + np.uint64(width) * row).astype(np.uint32)
