"""The bookkeeping of the frame store's two arenas (csrc/velo_block_list.h) as a stand-alone C++ program under the address and
undefined-behaviour sanitizers: the put / drop sequences of the GPU state tests replayed, and a seeded random sequence with the
invariants of the first-fit free list checked after every step (tests/cpp/test_block_list.cpp).  No GPU, no library."""
import os
import subprocess

from velo_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_block_list_under_sanitizers(tmp_path):
    exe = str(tmp_path / "test_block_list")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.dirname(build.LIB), os.path.join(CPP, "test_block_list.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] == "block list ok", out.stdout + out.stderr
