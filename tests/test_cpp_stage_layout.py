"""The layout of a staged buffer (csrc/velo_stage_layout.h) as a stand-alone C++ program under the address and undefined-behaviour
sanitizers: every count around a 64-byte boundary for element sizes that do not divide it, alignments 1 / 4 / 16 / 64, empty parts, every
element of every part written inside a heap block of exactly `bytes` bytes, and the offsets against the hand-written sums of three real
launch sets (tests/cpp/test_stage_layout.cpp).  No GPU, no library."""
import os
import subprocess

from velo_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_stage_layout_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_stage_layout")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.dirname(build.LIB), os.path.join(CPP, "test_stage_layout.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] == "stage layout ok", out.stdout + out.stderr
