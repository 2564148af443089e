"""velo_hip::PoseGraph::gateEdges, relativeCovariance and loopCandidates (include/velo_pose_graph.hpp): compile as C++11 against the header
alone (CPU); on the GPU the adaptor's results on fixture `chain5` equal, bit for bit, what the Python walk of the C-ABI gives."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pose_graph_ref as G
import pose_graph_weighted_ref as W
import velo_amd  # noqa: F401
from velo_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
PAIRS = ((0, 4), (1, 3), (4, 2), (0, 1))
QUERY = (4, 2)                                                         # the query frame and min_gap of the candidate list


def compile_driver(tmp_path) -> str:
    build.build_hip()
    exe = str(tmp_path / "test_pose_graph_gate")
    csrc = os.path.dirname(build.LIB)
    subprocess.run(["g++", "-std=c++11", "-pedantic", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(CPP, "test_pose_graph_gate.cpp"), "-o", exe, "-L", csrc, "-lvelo_hip", f"-Wl,-rpath,{csrc}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_adaptor_compiles_as_cxx11_and_links(tmp_path):
    out = subprocess.run([compile_driver(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and "pose graph gate adaptor linked" in out.stdout


def hex64(a):
    return " ".join(f"{v:016x}" for v in np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64))


def proposal(g):
    """a measurement and an information per pair of PAIRS: the true relative pose a little off, a random SPD W"""
    rng = np.random.default_rng(77)
    z = np.array([G.relative(g["truth"][a], g["truth"][b]) + np.concatenate([1e-3 * rng.normal(size=3), 0.02 * rng.normal(size=3)]) for a, b in PAIRS])
    w = np.array([W.info21(W.spd(rng, 100.0, 1e3)) for _ in PAIRS])
    return z, w


def write_case(path, g, z, w):
    frames = sorted(g["poses"])
    with open(path, "wb") as f:
        f.write(struct.pack("iiii", len(frames), len(g["edges"]), len(g["fixed"]), len(PAIRS)))
        f.write(np.asarray(frames, np.int32).tobytes())
        f.write(np.ascontiguousarray([g["poses"][k] for k in frames], np.float64).tobytes())
        f.write(np.asarray([e[0] for e in g["edges"]], np.int32).tobytes())
        f.write(np.asarray([e[1] for e in g["edges"]], np.int32).tobytes())
        f.write(np.ascontiguousarray([e[2] for e in g["edges"]], np.float64).tobytes())
        f.write(np.asarray([e[3] for e in g["edges"]], np.float64).tobytes())
        f.write(np.asarray(g["fixed"], np.int32).tobytes())
        f.write(np.asarray([p[0] for p in PAIRS], np.int32).tobytes())
        f.write(np.asarray([p[1] for p in PAIRS], np.int32).tobytes())
        f.write(np.ascontiguousarray(z, np.float64).tobytes())
        f.write(np.ascontiguousarray(w, np.float64).tobytes())
        f.write(np.asarray(QUERY, np.int32).tobytes())
    return frames


@pytest.mark.gpu
def test_adaptor_gives_the_c_abis_gate_of_chain5(tmp_path):
    exe = compile_driver(tmp_path)
    g = G.fixture("chain5")
    z, w = proposal(g)
    case = str(tmp_path / "graph.bin")
    frames = write_case(case, g, z, w)
    out = subprocess.run([exe, case], check=True, capture_output=True, text=True).stdout.splitlines()
    ctx = api.Context(0)
    ctx.graph_reset()
    for k in frames:
        ctx.graph_set_pose(k, g["poses"][k])
    for a, b, zz, info in g["edges"]:
        ctx.graph_add_edges([a], [b], [zz], [info])
    frm, to = [p[0] for p in PAIRS], [p[1] for p in PAIRS]
    rel, r, cov, chi2 = ctx.graph_edge_gate(frm, to, z, w, g["fixed"])
    rrel, rcov = ctx.graph_relative_covariance(np.asarray(PAIRS, dtype=np.int32), g["fixed"])
    cf, cd, cs = ctx.graph_loop_candidates(QUERY[0], QUERY[1], 3.5, 2.0, g["fixed"])
    ctx.close()
    assert np.all(chi2 > 0.0) and len(cf) >= 2 and np.all(cs > 0.0)
    for tag, arr in (("rel", rel), ("r", r), ("S", cov), ("chi2", chi2), ("rrel", rrel), ("rcov", rcov)):
        assert [line for line in out if line.startswith(tag + " ")] == [f"{tag} {p} {hex64(arr[p])}" for p in range(len(PAIRS))], tag
    assert [line for line in out if line.startswith("cand ")] == [f"cand {f} {hex64([d, s])}" for f, d, s in zip(cf, cd, cs)]
    assert out[-1] == "refused 1 optimizations 0"
