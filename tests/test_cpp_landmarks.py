"""The header-only C++ adaptor of the resident landmark store (include/velo_landmarks.hpp): compiles as C++11 against the stand-in
container types (CPU); on the GPU its `landmarks`, `keypoint_added` and `landmarks_at_frame` equal what the Python walk of the same
sequence gives."""
import os
import struct
import subprocess

import numpy as np
import pytest

import landmarks_ref as LR
import velo_amd  # noqa: F401
from velo_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def compile_driver(tmp_path) -> str:
    build.build_hip()
    exe = str(tmp_path / "test_landmarks")
    csrc = os.path.dirname(build.LIB)
    subprocess.run(["g++", "-std=c++11", "-pedantic", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CPP,
                    os.path.join(CPP, "test_landmarks.cpp"), "-o", exe, "-L", csrc, "-lvelo_hip", f"-Wl,-rpath,{csrc}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_adaptor_compiles_as_cxx11_and_links(tmp_path):
    out = subprocess.run([compile_driver(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and "landmarks adaptor linked" in out.stdout


@pytest.mark.gpu
def test_adaptor_equals_the_python_walk(tmp_path):
    exe = compile_driver(tmp_path)
    ids = list(range(0, 80))
    seq = LR.sequence(77, 8, 2, ids, first_frame={i: ((i * 3) % 8, 1 + (i * 5) % 6) for i in ids})
    at_frame, cap = 6, 24
    Minv = np.linalg.inv(api.pose_vec_to_mat(seq["poses"][at_frame]))
    case = str(tmp_path / "seq.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("iiii", 2, len(seq["poses"]), at_frame, cap))
        f.write(np.ascontiguousarray(seq["cam_trans"], np.float32).tobytes())
        f.write(np.ascontiguousarray(seq["poses"], np.float64).tobytes())
        f.write(np.ascontiguousarray(Minv, np.float64).tobytes())
        for per_cam in seq["frames"]:
            for i, k, h, c in per_cam:
                f.write(struct.pack("i", len(i)) + i.tobytes() + np.ascontiguousarray(k, np.float32).tobytes() + h.tobytes())
                f.write(struct.pack("i", len(c)) + np.ascontiguousarray(c, np.float32).tobytes())
    out = subprocess.run([exe, case], check=True, capture_output=True, text=True).stdout.splitlines()
    ctx = api.Context(0)
    ctx.landmarks_reset(seq["cam_trans"], log_capacity=cap)
    for fr in range(len(seq["poses"])):
        ctx.landmarks_set_pose(fr, seq["poses"][fr])
    for fr, per_cam in enumerate(seq["frames"]):
        for cam, (i, k, h, c) in enumerate(per_cam):
            ctx.landmarks_observe(fr, cam, i, k, h, c)
        ctx.landmarks_triangulate(fr)
    xyz, added, _ = ctx.landmarks_get(np.arange(ctx.landmarks_info()["n_ids"]))
    want_l = [f"l {i} " + " ".join(f"{v:08x}" for v in xyz[i].view(np.uint32)) for i in np.flatnonzero(added)]
    ai, ax = ctx.landmarks_at_frame(at_frame, Minv)
    want_a = [f"a {i} " + " ".join(f"{v:08x}" for v in p.view(np.uint32)) for i, p in zip(ai, ax)]
    ctx.close()
    assert len(want_l) > 30 and len(want_a) > 10
    assert [line for line in out if line.startswith("l ")] == want_l
    assert [line for line in out if line.startswith("a ")] == want_a
