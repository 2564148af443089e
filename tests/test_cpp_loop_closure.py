"""The loop-closure call site of the C++ adaptor (include/velo_frame_store.hpp: FrameStore::putDescriptors, frameToFrameLoop):
compiles as C++11 against the stand-in container types (CPU); on the GPU frameToFrameLoop equals frameToFrame fed with host-made
descriptor matches (velo_hip::matchFeatures) and a host landmarks_at_frame, on pose, matches, good_matches and residual_type."""
import os
import struct
import subprocess

import numpy as np
import pytest

import helpers as H
import loop_ref as LP
import velo_amd  # noqa: F401
from velo_amd import build, synth
from test_cpp_frame_store import frames_from_records

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def compile_driver(tmp_path) -> str:
    build.build_hip()
    exe = str(tmp_path / "test_loop_closure")
    csrc = os.path.dirname(build.LIB)
    subprocess.run(["g++", "-std=c++11", "-pedantic", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CPP,
                    os.path.join(CPP, "test_loop_closure.cpp"), "-o", exe, "-L", csrc, "-lvelo_hip", f"-Wl,-rpath,{csrc}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_adaptor_compiles_as_cxx11_and_links(tmp_path):
    out = subprocess.run([compile_driver(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and "loop closure adaptor linked" in out.stdout


@pytest.mark.gpu
def test_loop_registration_equals_the_host_made_one(tmp_path):
    exe = compile_driver(tmp_path)
    d = H.small_pair(16, 128)
    sides = frames_from_records(synth.stereo_matches(60, mix="all"), 4)
    desc = dict(zip((1, 0), LP.near_rows(np.random.default_rng(5), sides[1], sides[0])))
    want = sum(len(p) for p in LP.match_cameras(desc[1], desc[0])[0])
    assert 60 <= want < 120                                              # the filter keeps and drops
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
        for fr in (0, 1):
            for cam, rows in enumerate(desc[fr]):
                step = 64 if (cam + fr) % 2 else 80                      # every other matrix a ROI-like stride
                buf = np.full((len(rows), step), 0xA5, np.uint8)
                buf[:, :64] = rows
                f.write(struct.pack("ii", len(rows), step) + buf.tobytes())
        f.write(struct.pack("d", 29.0))
    out = subprocess.run([exe, case], check=True, capture_output=True, text=True).stdout.splitlines()
    counts = [int(v) for v in out[0].split()[1::2]]
    assert counts[0] == 2 * 69 and counts[1] == want and counts[2] > 0     # every keypoint of frame2 is a landmark
    assert out[1] == "loop equals host: 1"
