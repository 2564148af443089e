"""velo_hip::PoseGraph::covariance and jointCovariance (include/velo_pose_graph.hpp): compile as C++11 against the header alone, with the
call sites of before (CPU); on the GPU the adaptor's marginals of fixture `chain5` and one joint covariance equal, bit for bit, what
the Python walk of the C-ABI gives."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pose_graph_ref as G
import velo_amd  # noqa: F401
from velo_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
JOINT = (1, 4)


def compile_driver(tmp_path) -> str:
    build.build_hip()
    exe = str(tmp_path / "test_pose_graph_covariance")
    csrc = os.path.dirname(build.LIB)
    subprocess.run(["g++", "-std=c++11", "-pedantic", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(CPP, "test_pose_graph_covariance.cpp"), "-o", exe, "-L", csrc, "-lvelo_hip", f"-Wl,-rpath,{csrc}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_adaptor_compiles_as_cxx11_and_links(tmp_path):
    out = subprocess.run([compile_driver(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and "pose graph covariance adaptor linked" in out.stdout


def hex64(a):
    return " ".join(f"{v:016x}" for v in np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64))


def write_case(path, g):
    frames = sorted(g["poses"])
    with open(path, "wb") as f:
        f.write(struct.pack("iiii", len(frames), len(g["edges"]), len(g["fixed"]), 0))
        f.write(np.asarray(frames, np.int32).tobytes())
        f.write(np.ascontiguousarray([g["poses"][k] for k in frames], np.float64).tobytes())
        f.write(np.asarray([e[0] for e in g["edges"]], np.int32).tobytes())
        f.write(np.asarray([e[1] for e in g["edges"]], np.int32).tobytes())
        f.write(np.ascontiguousarray([e[2] for e in g["edges"]], np.float64).tobytes())
        f.write(np.asarray([e[3] for e in g["edges"]], np.float64).tobytes())
        f.write(np.asarray(g["fixed"], np.int32).tobytes())
        f.write(np.asarray(JOINT, np.int32).tobytes())
    return frames


@pytest.mark.gpu
def test_adaptor_gives_the_c_abis_covariances_of_chain5(tmp_path):
    exe = compile_driver(tmp_path)
    g = G.fixture("chain5")
    case = str(tmp_path / "graph.bin")
    frames = write_case(case, g)
    out = subprocess.run([exe, case], check=True, capture_output=True, text=True).stdout.splitlines()
    ctx = api.Context(0)
    ctx.graph_reset()
    for k in frames:
        ctx.graph_set_pose(k, g["poses"][k])
    for a, b, z, info in g["edges"]:
        ctx.graph_add_edges([a], [b], [z], [info])
    m = ctx.graph_covariance(frames, g["fixed"])
    J = ctx.graph_joint_covariance(JOINT[0], JOINT[1], g["fixed"])
    ctx.close()
    assert np.all(m[0] == 0.0) and all(np.all(np.diag(m[k]) > 0.0) for k in range(1, len(frames)))
    assert [line for line in out if line.startswith("m ")] == [f"m {f} {hex64(m[k])}" for k, f in enumerate(frames)]
    assert [line for line in out if line.startswith("j ")] == [f"j {JOINT[0]} {JOINT[1]} {hex64(J)}"]
    assert np.any(J[:6, 6:] != 0.0) and np.array_equal(J, J.T)
    assert out[-1] == "refused 1 optimizations 0"
