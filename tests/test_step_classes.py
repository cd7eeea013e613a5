"""The merged trace's host grouping (xraytracer_amd/csrc/host/step_classes.cpp: objects of equal
triangle count made contiguous, one class record per count) checked by a stand-alone program,
tests/cpp/step_classes_kat.cpp, which lists what it checks.  CPU only: g++ compiles the grouping and
the program together, once plainly and once with AddressSanitizer and UBSan, and each build runs
once."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xraytracer_amd", "csrc")


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")],
                         ids=["plain", "asan_ubsan"])
def test_step_classes_program(tmp_path, flags):
    exe = str(tmp_path / "step_classes_kat")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", *flags, "-I", os.path.join(ROOT, "include"), "-I", CSRC,
                           "-o", exe, os.path.join(ROOT, "tests", "cpp", "step_classes_kat.cpp"),
                           os.path.join(CSRC, "host", "step_classes.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr[-2000:])
