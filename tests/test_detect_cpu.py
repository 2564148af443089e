"""CPU checks of corner detection's boundary: velo_detect_features / velo_get_corner_response refuse unsupported arguments with the
library's usual argument error before any context is touched (no GPU needed), the defaults are the reference's constants, the ctypes
mirrors have the header's layout, and the C++ adaptor (include/velo_detect_features.hpp) compiles as C++11 against stand-in types."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import velo_amd  # noqa: F401
from velo_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return api.load_library()


def compile_detect_driver(tmp_path) -> str:
    build.build_hip()
    exe = str(tmp_path / "test_detect_features")
    csrc = os.path.dirname(build.LIB)
    subprocess.run(["g++", "-std=c++11", "-pedantic", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    "-I", CPP, os.path.join(CPP, "test_detect_features.cpp"), "-o", exe, "-L", csrc, "-lvelo_hip", f"-Wl,-rpath,{csrc}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_defaults_are_the_reference_constants(lib):
    p = api.VeloGfttParams()
    assert lib.velo_default_gftt_params(C.byref(p)) == 0
    assert (p.max_corners, p.block_size, p.quality_level, p.min_distance) == (3000, 3, 0.001, 12.0)   # kitti.h:7,18,19
    q = api.gftt_params()
    assert (q.max_corners, q.block_size, q.quality_level, q.min_distance) == (3000, 3, 0.001, 12.0)
    assert lib.velo_default_gftt_params(None) == -1
    assert C.sizeof(api.VeloGfttParams) == 24 and C.sizeof(api.VeloDetectJob) == 16       # the header's layout (LP64)


def test_argument_validation_without_gpu(lib):
    fake = C.c_void_p(0x1000)                       # never dereferenced: every argument is checked before the context is touched
    job = (api.VeloDetectJob * 1)()
    cnt = (C.c_int32 * 3)()
    xy, resp, fr = (C.c_float * 8)(), (C.c_float * 4)(), (C.c_uint8 * 4)()

    def call(p, jobs=job, n=1, cap=4, ctx=fake, a=xy, b=resp, c=fr, d=cnt):
        return lib.velo_detect_features(ctx, C.cast(jobs, C.c_void_p) if jobs is not None else None, n, C.byref(p) if p is not None else None,
                                        cap, a, b, c, d)
    ok = api.gftt_params()
    assert call(ok, ctx=None) == -1 and b"null ctx" in lib.velo_last_error()
    assert call(None) == -1 and b"null params" in lib.velo_last_error()
    assert call(ok, n=-1) == -1 and b"negative job count" in lib.velo_last_error()
    for bs in (1, 5, 7, 0):
        assert call(api.gftt_params(block_size=bs)) == -1 and b"block_size" in lib.velo_last_error()
    for md in (0.0, 0.99, 64.5, -3.0, float("nan"), float("inf")):
        assert call(api.gftt_params(min_distance=md)) == -1 and b"min_distance" in lib.velo_last_error(), md
    for q in (0.0, -0.1, 1.0001, float("nan")):
        assert call(api.gftt_params(quality_level=q)) == -1 and b"quality_level" in lib.velo_last_error(), q
    assert call(ok, cap=-1) == -1 and b"capacity" in lib.velo_last_error()
    assert call(ok, n=0) == 0                       # no job: nothing to do, nothing touched
    assert call(ok, jobs=None) == -1 and b"null jobs" in lib.velo_last_error()
    assert call(ok, d=None) == -1 and b"null counts" in lib.velo_last_error()
    assert call(ok, a=None) == -1 and b"null xy" in lib.velo_last_error()
    job[0].cam, job[0].n_existing = 0, -2
    assert call(ok) == -1 and b"negative point count" in lib.velo_last_error()
    job[0].n_existing = 5
    assert call(ok) == -1 and b"null points" in lib.velo_last_error()
    job[0].n_existing, job[0].cam = 0, 8
    assert call(ok) == -1 and b"camera 8" in lib.velo_last_error()
    job[0].cam = -1
    assert call(ok) == -1 and b"camera -1" in lib.velo_last_error()
    assert lib.velo_get_corner_response(None, 0, resp, 16) == -1
    assert lib.velo_get_corner_response(fake, 0, None, 16) == -1 and b"null out" in lib.velo_last_error()
    assert lib.velo_get_corner_response(fake, 0, resp, -1) == -1 and b"negative capacity" in lib.velo_last_error()


def test_python_wrapper_refuses_unknown_parameters():
    with pytest.raises(TypeError):
        api.gftt_params(use_harris=True)
    assert np.isclose(api.gftt_params(min_distance=12.4).min_distance, 12.4)


def test_cxx_adaptor_compiles_as_cxx11(tmp_path):
    assert os.path.exists(compile_detect_driver(tmp_path))
