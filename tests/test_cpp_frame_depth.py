"""FrameStore::putFrameWithDepth / putFramesWithDepth of the header-only C++ adaptor (include/velo_frame_store.hpp): compile as C++11
against the stand-in container types (CPU); on the GPU they leave the frame store and the landmark store equal to putFrame +
putDescriptors + LandmarkStore::observeFrame fed from velo_project_lidar + velo_depth_association, over three frames of two cameras."""
import os
import struct
import subprocess

import numpy as np
import pytest

import velo_amd  # noqa: F401
from velo_amd import build, synth
from test_depth_oracle import crafted_rings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def compile_driver(tmp_path) -> str:
    build.build_hip()
    exe = str(tmp_path / "test_frame_depth")
    csrc = os.path.dirname(build.LIB)
    subprocess.run(["g++", "-std=c++11", "-pedantic", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CPP,
                    os.path.join(CPP, "test_frame_depth.cpp"), "-o", exe, "-L", csrc, "-lvelo_hip", f"-Wl,-rpath,{csrc}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_adaptor_compiles_as_cxx11_and_links(tmp_path):
    out = subprocess.run([compile_driver(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and "frame depth adaptor linked" in out.stdout


@pytest.mark.gpu
def test_put_frame_with_depth_equals_todays_members(tmp_path):
    exe = compile_driver(tmp_path)
    xyz, off = crafted_rings(n_rings=150)
    w = synth.cam_window()
    rng = np.random.default_rng(70)
    sizes = [(300, 257), (520, 0), (256, 130)]                           # per frame: camera 0, camera 1 (one empty)
    case = str(tmp_path / "case.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("i", len(off) - 1) + np.asarray(off, np.int32).tobytes() + np.ascontiguousarray(xyz, np.float32).tobytes())
        f.write(struct.pack("iid", 2, len(sizes), 0.2))
        f.write(np.ascontiguousarray(synth.CAM_TRANS[:2], np.float32).tobytes() + np.concatenate([w, w]).astype(np.float64).tobytes())
        for fr, per_cam in enumerate(sizes):
            for cam, n in enumerate(per_cam):
                ids = rng.permutation(700)[:n].astype(np.int32)           # ids recur from frame to frame and between the cameras
                kps = synth.keypoints_in_window(n, seed=71 + 2 * fr + cam)
                f.write(struct.pack("i", n) + ids.tobytes() + np.ascontiguousarray(kps, np.float32).tobytes())
                f.write(rng.integers(0, 256, (n, 64), dtype=np.uint8).tobytes())
    out = subprocess.run([exe, case], check=True, capture_output=True, text=True).stdout.splitlines()
    n_kp, n_wd = [int(v) for v in out[0].split() if v.isdigit()]
    assert n_kp == sum(sum(s) for s in sizes) and 100 < n_wd < n_kp - 100      # both kinds
    assert out[1] == "putFrameWithDepth equals putFrame + putDescriptors + observeFrame: 1"
    assert out[2] == "putFramesWithDepth equals it on both contexts: 1 1"
