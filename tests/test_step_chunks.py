"""The block-owned chunks of the merged schedule's whole-wave phase (xraytracer_amd/csrc/step_chunks.h
and host/step_chunks.cpp: which block owns which chunk in which launch, how the partitions' live
entries become dense arrays, how many passes a launch runs and which renders take the phase) checked
by a stand-alone program, tests/cpp/step_chunks_kat.cpp, which lists what it checks.  CPU only: g++
compiles the map and the program together, once plainly and once with AddressSanitizer and UBSan,
and each build runs once."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "xraytracer_amd", "csrc")


@pytest.mark.parametrize("flags", [(), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")],
                         ids=["plain", "asan_ubsan"])
def test_step_chunks_program(tmp_path, flags):
    exe = str(tmp_path / "step_chunks_kat")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", *flags, "-I", CSRC, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "step_chunks_kat.cpp"),
                           os.path.join(CSRC, "host", "step_chunks.cpp")])
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", (run.returncode, run.stdout, run.stderr[-2000:])
