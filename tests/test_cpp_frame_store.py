"""The header-only C++ adaptor of the resident keypoint frames (include/velo_frame_store.hpp): compiles as C++11 against the stand-in
container types (CPU); on the GPU frameToFrameResident equals frameToFrame fed with host-made matches and landmarks_at_frame, on
pose, matches, good_matches and residual_type."""
import os
import struct
import subprocess

import numpy as np
import pytest

import helpers as H
import velo_amd  # noqa: F401
from velo_amd import api, build, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def compile_driver(tmp_path) -> str:
    build.build_hip()
    exe = str(tmp_path / "test_frame_store")
    csrc = os.path.dirname(build.LIB)
    subprocess.run(["g++", "-std=c++11", "-pedantic", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CPP,
                    os.path.join(CPP, "test_frame_store.cpp"), "-o", exe, "-L", csrc, "-lvelo_hip", f"-Wl,-rpath,{csrc}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_adaptor_compiles_as_cxx11_and_links(tmp_path):
    out = subprocess.run([compile_driver(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and "frame store adaptor linked" in out.stdout


def frames_from_records(rec, seed):
    """frame 1 (frame1) and frame 0 (frame2), 2 cameras, whose id join gives the records of synth.stereo_matches back: shuffled
    keypoint order, distinct ids, and keypoints on either side that match nothing"""
    rng = np.random.default_rng(seed)
    m = api.matches_from_dict(rec)
    sides = {0: [], 1: []}
    for cam in range(2):
        r = m[m["cam"] == cam]
        n, extra = len(r), 9
        for fr, kp, p3, d, lo in ((1, r["p2_1"], r["p3_1"], r["d1"], 10000), (0, r["p2_2"], r["p3_2"], r["d2"], 20000)):
            ids = np.r_[1000 * cam + np.arange(n), lo + 100 * cam + np.arange(extra)].astype(np.int32)   # distinct per camera
            kps = np.vstack([kp, rng.normal(size=(extra, 2)) * .2]).astype(np.float32)
            with_depth = np.flatnonzero(np.r_[d != 0, np.zeros(extra, bool)])
            has = np.full(n + extra, -1, dtype=np.int32)
            slot = rng.permutation(len(with_depth))
            has[with_depth] = slot
            cloud = np.zeros((len(with_depth), 3), dtype=np.float32)
            cloud[slot] = p3[with_depth]
            perm = rng.permutation(n + extra)
            sides[fr].append((ids[perm], kps[perm], has[perm], cloud))
    return sides


@pytest.mark.gpu
def test_resident_registration_equals_the_host_made_one(tmp_path):
    exe = compile_driver(tmp_path)
    d = H.small_pair(16, 128)
    sides = frames_from_records(synth.stereo_matches(60, mix="all"), 4)
    case = str(tmp_path / "case.bin")
    with open(case, "wb") as f:
        for xyz, off in ((d["src_xyz"], d["src_off"]), (d["tgt_xyz"], d["tgt_off"])):
            f.write(struct.pack("i", len(off) - 1))
            f.write(np.asarray(off, np.int32).tobytes())
            f.write(np.ascontiguousarray(np.asarray(xyz, np.float32)[:, :3]).tobytes())
        f.write(struct.pack("ii", 2, 2))
        f.write(np.asarray(d["x0"], np.float64).tobytes())
        f.write(np.ascontiguousarray(synth.CAM_TRANS[:2], np.float32).tobytes())
        for fr in (0, 1):
            for i, k, h, c in sides[fr]:
                f.write(struct.pack("i", len(i)) + i.tobytes() + np.ascontiguousarray(k, np.float32).tobytes() + h.tobytes())
                f.write(struct.pack("i", len(c)) + np.ascontiguousarray(c, np.float32).tobytes())
    out = subprocess.run([exe, case], check=True, capture_output=True, text=True).stdout.splitlines()
    counts = [int(v) for v in out[0].split()[1::2]]
    assert counts[0] == 2 * 69 and counts[1] == 120 and counts[2] > 0        # every keypoint of frame2 is a landmark; 60 matches per camera
    assert out[1] == "resident equals host: 1"
