"""The owner of the host side's runtime handles (template Owned in csrc/velo_host_types.inl) as a stand-alone C++ program under the
address and undefined-behaviour sanitizers, with a test handle and a counting destroy function: move, move-assignment over a live
handle, self-move, reset, put() and the vector operations its holders perform (tests/cpp/test_owned.cpp).  The template's text is cut
out of the .inl, so the program compiles what the library compiles.  No GPU, no library."""
import os
import re
import subprocess

from velo_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def test_owner_under_sanitizers(tmp_path):
    text = open(os.path.join(build.CSRC, "velo_host_types.inl")).read()
    m = re.search(r"^template <typename H, auto Destroy>\nstruct Owned \{\n.*?^\};\n", text, re.S | re.M)
    assert m, "template Owned not found in velo_host_types.inl"
    (tmp_path / "owned_slice.h").write_text(m.group(0))
    exe = str(tmp_path / "test_owned")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", str(tmp_path), os.path.join(CPP, "test_owned.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.splitlines()[-1] == "owner ok", out.stdout + out.stderr
