"""velo_hip::PoseGraph::optimize with its solver argument (include/velo_pose_graph.hpp): compiles as C++11 against the header alone,
with the call sites of before the argument (CPU); on the GPU it optimises fixture `chain5` with the envelope solver and leaves the
poses and the summary equal, bit for bit, to what the Python walk of the C-ABI gives with linear_solver="envelope"."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pose_graph_env_fixtures as F
import pose_graph_ref as G
import velo_amd  # noqa: F401
from velo_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def compile_driver(tmp_path) -> str:
    build.build_hip()
    exe = str(tmp_path / "test_pose_graph_envelope")
    csrc = os.path.dirname(build.LIB)
    subprocess.run(["g++", "-std=c++11", "-pedantic", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(CPP, "test_pose_graph_envelope.cpp"), "-o", exe, "-L", csrc, "-lvelo_hip", f"-Wl,-rpath,{csrc}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_adaptor_compiles_as_cxx11_and_links(tmp_path):
    out = subprocess.run([compile_driver(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and "pose graph envelope adaptor linked" in out.stdout


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
    return frames


@pytest.mark.gpu
def test_adaptor_optimises_chain5_with_the_envelope_solver_like_the_c_abi(tmp_path):
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
    s = ctx.graph_optimize(g["fixed"], linear_solver="envelope")
    poses = {k: ctx.graph_get_poses(k, 1)[0] for k in frames}
    info = ctx.graph_info()
    ctx.close()
    assert s.iterations >= 2 and s.n_edges == len(g["edges"])
    want_s = f"s {s.termination} {s.iterations} {s.evaluations} {s.n_nodes} {s.n_free} {s.n_edges} {s.n_trace} {hex64([s.initial_cost, s.final_cost])}"
    want_t = [f"t {s.trace[k].iteration} {s.trace[k].status} 0 {hex64([s.trace[k].cost, s.trace[k].candidate_cost])}" for k in range(s.n_trace)]
    want_p = [f"p {k} {hex64(poses[k])}" for k in frames]
    assert out[0] == want_s
    assert [line for line in out if line.startswith("t ")] == want_t
    assert [line for line in out if line.startswith("p ")] == want_p
    assert any(not np.array_equal(poses[k], g["poses"][k]) for k in frames[1:]) and np.array_equal(poses[0], g["poses"][0])
    n, ea, eb = F.free_graph(g)
    _, _, stats = api.graph_order(n, ea, eb)
    assert (info["envelope_widest_row"], info["envelope_blocks"]) == (stats["widest_row"], stats["envelope_blocks"])
    assert out[-1] == f"refused 1 kept 1 envelope {stats['widest_row']} {stats['envelope_blocks']}"
