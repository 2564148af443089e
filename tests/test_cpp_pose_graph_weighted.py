"""velo_hip::PoseGraph's weighted members -- addEdgeWeighted, addRegistration, edgeStats (include/velo_pose_graph.hpp): compile as
C++11 against the header alone (CPU); on the GPU addRegistration + optimize + edgeStats on fixture `chain5_mixed` leave the poses, the
summary and the edges' figures equal, bit for bit, to what the Python walk of the C-ABI gives."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pose_graph_weighted_ref as W
import velo_amd  # noqa: F401
from velo_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def compile_driver(tmp_path) -> str:
    build.build_hip()
    exe = str(tmp_path / "test_pose_graph_weighted")
    csrc = os.path.dirname(build.LIB)
    subprocess.run(["g++", "-std=c++11", "-pedantic", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(CPP, "test_pose_graph_weighted.cpp"), "-o", exe, "-L", csrc, "-lvelo_hip", f"-Wl,-rpath,{csrc}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_adaptor_compiles_as_cxx11_and_links(tmp_path):
    out = subprocess.run([compile_driver(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and "pose graph weighted adaptor linked" in out.stdout


def hex64(a):
    return " ".join(f"{v:016x}" for v in np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64))


@pytest.mark.gpu
def test_adaptor_adds_registrations_and_reads_edge_stats_like_the_c_abi(tmp_path):
    exe = compile_driver(tmp_path)
    g = W.fixture("chain5_mixed")
    scalar = [e for e in g["edges"] if np.ndim(e[3]) == 0]
    regs = [e for e in g["edges"] if np.ndim(e[3]) == 2]              # the fixture's 6 x 6 serves as the registration's JtJ here
    assert g["edges"] == scalar + regs and len(regs) == 1 and regs[0][4] > 0.0
    frames = sorted(g["poses"])
    case = str(tmp_path / "graph.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("iiii", len(frames), len(scalar), len(g["fixed"]), len(regs)))
        f.write(np.asarray(frames, np.int32).tobytes())
        f.write(np.ascontiguousarray([g["poses"][k] for k in frames], np.float64).tobytes())
        f.write(np.asarray([e[0] for e in scalar], np.int32).tobytes())
        f.write(np.asarray([e[1] for e in scalar], np.int32).tobytes())
        f.write(np.ascontiguousarray([e[2] for e in scalar], np.float64).tobytes())
        f.write(np.asarray([e[3] for e in scalar], np.float64).tobytes())
        f.write(np.asarray(g["fixed"], np.int32).tobytes())
        f.write(np.asarray([e[0] for e in regs], np.int32).tobytes())
        f.write(np.asarray([e[1] for e in regs], np.int32).tobytes())
        f.write(np.ascontiguousarray([e[2] for e in regs], np.float64).tobytes())
        f.write(np.ascontiguousarray([e[3] for e in regs], np.float64).tobytes())
        f.write(np.asarray([e[4] for e in regs], np.float64).tobytes())
    out = subprocess.run([exe, case], check=True, capture_output=True, text=True).stdout.splitlines()
    ctx = api.Context(0)
    ctx.graph_reset()
    for k in frames:
        ctx.graph_set_pose(k, g["poses"][k])
    for a, b, z, info, _ in scalar:
        ctx.graph_add_edges([a], [b], [z], [info])
    for a, b, z, H, loss in regs:
        ctx.graph_add_edges_weighted([a], [b], [z], [api.graph_edge_information(z, H)], [loss])
    s = ctx.graph_optimize(g["fixed"])
    poses = {k: ctx.graph_get_poses(k, 1)[0] for k in frames}
    chi2, weight = ctx.graph_edge_stats()
    ctx.close()
    assert s.iterations >= 2 and s.n_edges == len(g["edges"]) and 0.0 < weight[-1] < 1.0
    want_s = f"s {s.termination} {s.iterations} {s.evaluations} {s.n_nodes} {s.n_free} {s.n_edges} {s.n_trace} {hex64([s.initial_cost, s.final_cost])}"
    want_t = [f"t {s.trace[k].iteration} {s.trace[k].status} {s.trace[k].cg_iterations} {hex64([s.trace[k].cost, s.trace[k].candidate_cost])}" for k in range(s.n_trace)]
    assert out[0] == want_s
    assert [line for line in out if line.startswith("t ")] == want_t
    assert [line for line in out if line.startswith("p ")] == [f"p {k} {hex64(poses[k])}" for k in frames]
    assert [line for line in out if line.startswith("e ")] == [f"e {k} {hex64([chi2[k], weight[k]])}" for k in range(len(chi2))]
    assert out[-1] == "refused 1 kept 1"
