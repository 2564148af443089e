"""CPU checks of the feature-tracking C++ adaptor (include/velo_track_features.hpp): it compiles as C++11 against the stand-in types
(tests/cpp/track_standin.hpp), and its consolidateFeatures (velo.h:179-230, host code) gives the lists of the restatement
(tests/lk_ref.py consolidate) bit for bit on crafted input: pairs, three or more entries (geomedian), a coincident point, id order."""
import os
import struct
import subprocess

import numpy as np

import lk_ref as R
import velo_amd  # noqa: F401
from velo_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1]], np.float32)


def compile_track_driver(tmp_path) -> str:
    build.build_hip()
    exe = str(tmp_path / "test_track_features")
    csrc = os.path.dirname(build.LIB)
    subprocess.run(["g++", "-std=c++11", "-pedantic", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    "-I", CPP, os.path.join(CPP, "test_track_features.cpp"), "-o", exe, "-L", csrc, "-lvelo_hip", f"-Wl,-rpath,{csrc}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def parse_lists(out):
    """{name: [values, ...] per occurrence}; point lists come back as float32 [n, 2], descriptor lists as uint8 bytes"""
    res = {}
    for line in out.strip().splitlines():
        parts = line.split()
        name, n, vals = parts[0], int(parts[1]), np.asarray(parts[2:], np.int64)
        if name.endswith(("_k", "_p")):
            v = vals.astype(np.uint32).view(np.float32).reshape(n, 2)
        elif name.endswith("_d"):
            v = vals.astype(np.uint8)
        else:
            v = vals
        res.setdefault(name, []).append(v)
    return res


def check_lists(got, prefix, i, want):
    kp, kp_p, ids, desc = want
    assert np.array_equal(got[prefix + "_k"][i].view(np.uint32), np.asarray(kp, np.float32).reshape(-1, 2).view(np.uint32)), (prefix, i)
    assert np.array_equal(got[prefix + "_p"][i].view(np.uint32), np.asarray(kp_p, np.float32).reshape(-1, 2).view(np.uint32)), (prefix, i)
    assert got[prefix + "_id"][i].tolist() == list(ids), (prefix, i)
    assert np.array_equal(got[prefix + "_d"][i], np.asarray(desc, np.uint8).reshape(-1)), (prefix, i)


def test_cxx_consolidate_equals_the_restatement(tmp_path):
    exe = compile_track_driver(tmp_path)
    rng = np.random.default_rng(3)
    kp = rng.normal(0, 0.3, (40, 2)).astype(np.float32)
    ids = [9, 2, 9, 4, 2, 7, 7, 7, 5, 5, 5, 5, 1, 3, 3, 8, 8, 8]        # singles, pairs, triples, a quadruple; out of order
    ids += list(rng.integers(0, 12, 22))
    kp[10] = kp[9]                                                    # id 5: two of its four entries coincide
    kp[15] = kp[16] = kp[17] = np.array([0.1, -0.2], np.float32)      # id 8: all coincident, the eps early return
    desc = rng.integers(0, 256, (40, 8), dtype=np.uint8)
    case = str(tmp_path / "cons.bin")
    with open(case, "wb") as f:
        f.write(K.astype(np.float32).tobytes())
        f.write(struct.pack("i", len(kp)))
        f.write(kp.tobytes())
        f.write(np.asarray(ids, np.int32).tobytes())
        f.write(struct.pack("i", 8))
        f.write(desc.tobytes())
    out = subprocess.run([exe, case, "consolidate"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = parse_lists(out.stdout)
    want = R.consolidate(kp, ids, desc, K)
    assert list(want[2]) == sorted(set(ids))
    assert max(ids.count(i) for i in set(ids)) > 2
    check_lists(got, "cons", 0, want)
