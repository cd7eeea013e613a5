"""The slot -> pixel map (xraytracer_amd/csrc/slot_map.h and host/slot_map.cpp: which pixel a path
slot renders, and the multiplier that interleaves them) checked by a stand-alone program,
tests/cpp/slot_map_kat.cpp, which lists what it checks.  CPU only: g++ compiles the map and the
program together, once plainly and once with AddressSanitizer and UBSan, and each build runs once.
The plain build also prints the map of two images for tests/slot_map_restatement.py, the Python
restatement the GPU tests compare the device's map with."""
import os
import subprocess

import numpy as np
import pytest

from slot_map_restatement import multiplier, pixels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xraytracer_amd", "csrc")


def build(tmp_path, flags=()):
    exe = str(tmp_path / "slot_map_kat")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", *flags, "-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "slot_map_kat.cpp"),
                           os.path.join(CSRC, "host", "slot_map.cpp")])
    return exe


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")],
                         ids=["plain", "asan_ubsan"])
def test_slot_map_program(tmp_path, flags):
    run = subprocess.run([build(tmp_path, flags)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr[-2000:])


def test_restatement_is_the_program(tmp_path):
    exe = build(tmp_path)
    for w, h in ((800, 600), (37, 29)):
        run = subprocess.run([exe, "dump", str(w), str(h)], capture_output=True, text=True, check=True)
        got = np.array(run.stdout.split(), dtype=np.uint32)
        assert np.array_equal(got, pixels(w, h)), (w, h)
    assert multiplier(1) == 0 and multiplier(2) == 1 and multiplier(480000) == 183347   # 183344..6 share 2, 3 or 5 with 2^8 3 5^4
    p = pixels(64, 96, shard_index=3, shard_count=8)
    assert sorted(p.tolist()) == [c + 64 * r for r in range(3, 96, 8) for c in range(64)]
    assert np.array_equal(pixels(5, 3, interleave=False), np.arange(15, dtype=np.uint32))
