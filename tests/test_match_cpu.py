"""CPU checks of descriptor matching (velo_match_descriptors, include/velo_match_features.hpp): the entry point refuses bad
arguments before it touches a device, the C++ adaptor compiles as C++11 against the stand-in matrix, and its host-only part
(matchUsingId, velo.h:562-590) gives the reference's pairs."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

import velo_amd  # noqa: F401
from velo_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def compile_driver(tmp_path) -> str:
    build.build_hip()
    exe = str(tmp_path / "test_match_features")
    csrc = os.path.dirname(build.LIB)
    subprocess.run(["g++", "-std=c++11", "-pedantic", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-I", CPP,
                    os.path.join(CPP, "test_match_features.cpp"), "-o", exe, "-L", csrc, "-lvelo_hip", f"-Wl,-rpath,{csrc}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def write_case(path, desc, ids, strides=None):
    """desc[cam][frame]: uint8 (n, 64); ids[cam][frame]: int list; strides[cam][frame]: row stride of the stand-in (>= 64)"""
    with open(path, "wb") as f:
        f.write(struct.pack("ii", len(desc), len(desc[0])))
        for c, per in enumerate(desc):
            for fr, d in enumerate(per):
                step = strides[c][fr] if strides else 64
                f.write(struct.pack("ii", len(d), step))
                buf = np.zeros((len(d), step), np.uint8)
                buf[:, :64] = d
                buf[:, 64:] = 0xA5                                  # padding the adaptor must not read as descriptor bits
                f.write(buf.tobytes())
        for per in ids:
            for v in per:
                f.write(struct.pack("i", len(v)))
                f.write(np.asarray(v, np.int32).tobytes())


def parse(out):
    rows = []
    for line in out.strip().splitlines():
        parts = line.split()
        n = int(parts[1])
        rows.append((parts[0], np.asarray(parts[2:], np.int64).reshape(n, 2)))
    return rows


def match_using_id(ids1, ids2):
    """velo.h:569-578"""
    id2ind = {}
    for ind, i in enumerate(ids1):
        id2ind[i] = ind
    return [(id2ind[i], ind) for ind, i in enumerate(ids2) if i in id2ind]


def test_entry_point_refuses_bad_arguments_without_a_device():
    build.build_hip()
    lib = api.load_library()
    fake = C.c_void_p(0x1000)                                   # never dereferenced: every check comes first
    buf = (C.c_int32 * 64)()
    ok = api.VeloDescJob(C.c_void_p(0x2000), 2, C.c_void_p(0x3000), 3)
    one = (api.VeloDescJob * 1)(ok)
    assert lib.velo_match_descriptors(None, one, 1, 29.0, buf, buf, buf, buf, buf) == -1 and b"null ctx" in lib.velo_last_error()
    assert lib.velo_match_descriptors(fake, one, -1, 29.0, buf, buf, buf, buf, buf) == -1 and b"negative job count" in lib.velo_last_error()
    assert lib.velo_match_descriptors(fake, None, 0, 29.0, None, None, None, None, None) == 0        # nothing to do
    assert lib.velo_match_descriptors(fake, None, 1, 29.0, buf, buf, buf, buf, buf) == -1
    for bad in (api.VeloDescJob(C.c_void_p(0x2000), -1, C.c_void_p(0x3000), 3), api.VeloDescJob(C.c_void_p(0x2000), 2, C.c_void_p(0x3000), -4)):
        arr = (api.VeloDescJob * 1)(bad)
        assert lib.velo_match_descriptors(fake, arr, 1, 29.0, buf, buf, buf, buf, buf) == -1 and b"negative size" in lib.velo_last_error()
    for bad in (api.VeloDescJob(None, 2, C.c_void_p(0x3000), 3), api.VeloDescJob(C.c_void_p(0x2000), 2, None, 3)):
        arr = (api.VeloDescJob * 1)(bad)
        assert lib.velo_match_descriptors(fake, arr, 1, 29.0, buf, buf, buf, buf, buf) == -1 and b"null descriptor rows" in lib.velo_last_error()
    big = (api.VeloDescJob * 1)(api.VeloDescJob(C.c_void_p(0x2000), 2, C.c_void_p(0x3000), (1 << 22) + 1))
    assert lib.velo_match_descriptors(fake, big, 1, 29.0, buf, buf, buf, buf, buf) == -1 and b"indexes at most" in lib.velo_last_error()
    assert lib.velo_match_descriptors(fake, one, 1, 29.0, None, buf, buf, buf, buf) == -1
    assert lib.velo_match_descriptors(fake, one, 1, 29.0, buf, buf, None, buf, buf) == -1
    assert lib.velo_match_descriptors(fake, one, 1, 29.0, buf, buf, buf, buf, None) == -1
    assert lib.velo_match_descriptors(fake, one, 1, float("nan"), buf, buf, buf, buf, buf) == -1


def test_cxx_adaptor_compiles_and_matches_by_id_on_the_host(tmp_path):
    """include/velo_match_features.hpp builds as C++11 against tests/cpp/mat_standin.hpp; matchUsingId (host code) equals velo.h:562-590"""
    exe = compile_driver(tmp_path)
    rng = np.random.default_rng(0)
    desc = [[rng.integers(0, 256, (5, 64), dtype=np.uint8) for _ in range(3)] for _ in range(2)]
    ids = [[list(rng.choice(20, size=12, replace=True)) for _ in range(3)] for _ in range(2)]   # repeats: the last index wins
    case = str(tmp_path / "case.bin")
    write_case(case, desc, ids)
    out = subprocess.run([exe, case, "ids"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    rows = parse(out.stdout)
    assert [r[0] for r in rows] == ["id_cam01", "id_frame", "id_frame"]
    assert rows[0][1].tolist() == [list(p) for p in match_using_id(ids[0][0], ids[1][1])]
    for c in range(2):
        assert rows[1 + c][1].tolist() == [list(p) for p in match_using_id(ids[c][0], ids[c][2])]
