"""LandmarkStore::bundleAdjust of the header-only C++ adaptor (include/velo_landmarks.hpp): compiles as C++11 against the stand-in
container types (CPU); on the GPU it walks fixture B of the bundle adjustment tests and leaves ceres_poses_vec, landmarks and the
summary equal, bit for bit, to what the Python walk of the C-ABI gives."""
import os
import struct
import subprocess

import numpy as np
import pytest

import ba_ref as B
import velo_amd  # noqa: F401
from velo_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def compile_driver(tmp_path) -> str:
    build.build_hip()
    exe = str(tmp_path / "test_bundle_adjust")
    csrc = os.path.dirname(build.LIB)
    subprocess.run(["g++", "-std=c++11", "-pedantic", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CPP,
                    os.path.join(CPP, "test_bundle_adjust.cpp"), "-o", exe, "-L", csrc, "-lvelo_hip", f"-Wl,-rpath,{csrc}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_adaptor_compiles_as_cxx11_and_links(tmp_path):
    out = subprocess.run([compile_driver(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and "bundle adjust adaptor linked" in out.stdout


def hex64(a):
    return " ".join(f"{v:016x}" for v in np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64))


@pytest.mark.gpu
def test_adaptor_walks_fixture_b_like_the_c_abi(tmp_path):
    exe = compile_driver(tmp_path)
    seq = B.fixture_sequence("B")
    F = len(seq["poses"])
    case = str(tmp_path / "seq.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("iii", 2, F, 1))
        f.write(np.ascontiguousarray(seq["cam_trans"], np.float32).tobytes())
        f.write(np.ascontiguousarray(seq["poses"], np.float64).tobytes())
        for per_cam in seq["frames"]:
            for i, k, h, c in per_cam:
                f.write(struct.pack("i", len(i)) + i.tobytes() + np.ascontiguousarray(k, np.float32).tobytes() + h.tobytes())
                f.write(struct.pack("i", len(c)) + np.ascontiguousarray(c, np.float32).tobytes())
    out = subprocess.run([exe, case], check=True, capture_output=True, text=True).stdout.splitlines()
    ctx = api.Context(0)
    ctx.landmarks_reset(seq["cam_trans"])
    for fr in range(F):
        ctx.landmarks_set_pose(fr, seq["poses"][fr])
    for fr, per_cam in enumerate(seq["frames"]):
        for cam, (i, k, h, c) in enumerate(per_cam):
            ctx.landmarks_observe(fr, cam, i, k, h, c)
        ctx.landmarks_triangulate(fr)
    poses, s = ctx.landmarks_adjust(list(range(F)), 1)
    xyz, added, _ = ctx.landmarks_get(np.arange(ctx.landmarks_info()["n_ids"]))
    ctx.close()
    assert s.iterations > 10 and s.n_landmarks == 40
    want_s = f"s {s.termination} {s.iterations} {s.evaluations} {s.n_landmarks} {s.n_blocks} {s.n_residuals} {s.n_trace} {hex64([s.initial_cost, s.final_cost])}"
    want_t = [f"t {s.trace[k].iteration} {s.trace[k].status} {hex64([s.trace[k].cost, s.trace[k].candidate_cost])}" for k in range(s.n_trace)]
    want_p = [f"p {fr} {hex64(poses[fr])}" for fr in range(F)]
    want_l = [f"l {i} " + " ".join(f"{v:08x}" for v in xyz[i].view(np.uint32)) for i in np.flatnonzero(added)]
    assert out[0] == want_s
    assert [line for line in out if line.startswith("t ")] == want_t
    assert [line for line in out if line.startswith("p ")] == want_p
    assert [line for line in out if line.startswith("l ")] == want_l
    assert not np.array_equal(poses[1:], seq["poses"][1:]) and np.array_equal(poses[0], seq["poses"][0])
    assert out[-1] == "refused 1 kept 1"
