"""velo_hip::PoseGraph::retain, release and retained (include/velo_pose_graph.hpp): compile as C++11 against the header alone (CPU); on
the GPU fixture `chain5` grown from 3 frames to 5 through the adaptor gives, bit for bit, what the Python walk of the C-ABI gives."""
import os
import struct
import subprocess

import numpy as np
import pytest

import pose_graph_retained_cases as K
import velo_amd  # noqa: F401
from velo_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def compile_driver(tmp_path) -> str:
    build.build_hip()
    exe = str(tmp_path / "test_pose_graph_retained")
    csrc = os.path.dirname(build.LIB)
    subprocess.run(["g++", "-std=c++11", "-pedantic", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(CPP, "test_pose_graph_retained.cpp"), "-o", exe, "-L", csrc, "-lvelo_hip", f"-Wl,-rpath,{csrc}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_adaptor_compiles_as_cxx11_and_links(tmp_path):
    out = subprocess.run([compile_driver(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and "pose graph retained adaptor linked" in out.stdout


def hex64(a):
    return " ".join(f"{v:016x}" for v in np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64))


def write_case(path, g, st):
    frames = [(f, s) for s, (grp, _) in enumerate(st) for f in grp]
    edges = [(e, s) for s, (_, es) in enumerate(st) for e in es]
    with open(path, "wb") as f:
        f.write(struct.pack("iiii", len(frames), len(edges), len(g["fixed"]), len(st)))
        f.write(np.asarray([k for k, _ in frames], np.int32).tobytes())
        f.write(np.asarray([s for _, s in frames], np.int32).tobytes())
        f.write(np.ascontiguousarray([g["poses"][k] for k, _ in frames], np.float64).tobytes())
        f.write(np.asarray([e[0] for e, _ in edges], np.int32).tobytes())
        f.write(np.asarray([e[1] for e, _ in edges], np.int32).tobytes())
        f.write(np.asarray([s for _, s in edges], np.int32).tobytes())
        f.write(np.ascontiguousarray([e[2] for e, _ in edges], np.float64).tobytes())
        f.write(np.asarray([e[3] for e, _ in edges], np.float64).tobytes())
        f.write(np.asarray(g["fixed"], np.int32).tobytes())


@pytest.mark.gpu
def test_adaptor_gives_the_c_abis_bits_on_chain5_grown_from_3_to_5(tmp_path):
    exe = compile_driver(tmp_path)
    g, st = K.stages("chain5")
    case = str(tmp_path / "graph.bin")
    write_case(case, g, st)
    out = subprocess.run([exe, case], check=True, capture_output=True, text=True).stdout.splitlines()
    ctx = api.Context(0)
    ctx.graph_reset()
    want, posed = [], []
    for s, (frames, edges) in enumerate(st):
        for k in frames:
            ctx.graph_set_pose(k, g["poses"][k])
            posed.append(k)
        for a, b, zz, info in edges:
            ctx.graph_add_edges([a], [b], [zz], [info])
        if s == 0:
            ctx.graph_retain(g["fixed"])
        cov = ctx.graph_covariance(np.asarray(posed, np.int32), g["fixed"])
        want += [f"cov {s} {k} {hex64(cov[p])}" for p, k in enumerate(posed)]
        rel, rcov = ctx.graph_relative_covariance(np.asarray([[posed[1], posed[-1]]], np.int32), g["fixed"])
        want += [f"rel {s} {posed[-1]} {hex64(rel[0])}", f"rcov {s} {posed[-1]} {hex64(rcov[0])}"]
    info = ctx.graph_retained()
    ctx.close()
    assert len(st) == 3 and [len(grp) for grp, _ in st] == [3, 1, 1] and info["extensions"] == 2 and info["builds"] == 1
    want.append(f"retained state 1 free {info['n_free']} builds 1 extensions 2 rebuilds {info['rebuilds']} served {info['served']} perm " + " ".join(str(v) for v in info["perm"]))
    want.append("released state 0")
    assert out == want
