"""The partition groups of the merged schedule's step launches (xraytracer_amd/csrc/step_groups.h and
host/step_groups.cpp: which partitions a group's launch serves, and when a render may run in
groups) checked by a stand-alone program, tests/cpp/step_groups_kat.cpp, which lists what it checks.
CPU only: g++ compiles the mapping and the program together, once plainly and once with
AddressSanitizer and UBSan, and each build runs once."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xraytracer_amd", "csrc")


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")],
                         ids=["plain", "asan_ubsan"])
def test_step_groups_program(tmp_path, flags):
    exe = str(tmp_path / "step_groups_kat")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", *flags, "-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "step_groups_kat.cpp"),
                           os.path.join(CSRC, "host", "step_groups.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr[-2000:])
