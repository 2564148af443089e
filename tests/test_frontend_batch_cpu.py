"""CPU checks of the batched visual front end's boundary: velo_set_images_batch / velo_track_features_batch /
velo_detect_features_batch refuse unsupported arguments with the library's usual argument error before any context is touched (no GPU
needed: the fake contexts are never dereferenced), the Python wrappers refuse unknown parameters, and the batch members of the C++
adaptors (include/velo_track_features.hpp, include/velo_detect_features.hpp) compile as C++11 against the stand-in types."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import velo_amd  # noqa: F401
from velo_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


def compile_frontend_batch_driver(tmp_path) -> str:
    build.build_hip()
    exe = str(tmp_path / "test_frontend_batch")
    csrc = os.path.dirname(build.LIB)
    subprocess.run(["g++", "-std=c++11", "-pedantic", "-O1", "-Wall", "-Werror", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                    "-I", CPP, os.path.join(CPP, "test_frontend_batch.cpp"), "-o", exe, "-L", csrc, "-lvelo_hip", f"-Wl,-rpath,{csrc}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return api.load_library()


def handles(*addr):
    return (C.c_void_p * len(addr))(*addr)


def check_context_list(lib, call):
    """the checks every batch entry makes on (ctxs, n_ctx) first; call(ctxs, n_ctx) -> status"""
    two = handles(0x1000, 0x2000)
    assert call(None, 2) == -1 and b"null context list" in lib.velo_last_error()
    assert call(two, 0) == -1 and b"0 contexts" in lib.velo_last_error()
    assert call(two, -3) == -1 and b"-3 contexts" in lib.velo_last_error()
    assert call(two, 257) == -1 and b"257 contexts" in lib.velo_last_error()
    assert call(handles(0x1000, 0), 2) == -1 and b"context 1 is null" in lib.velo_last_error()
    assert call(handles(0x1000, 0x2000, 0x1000), 3) == -1 and b"entries 0 and 2 are the same context" in lib.velo_last_error()


def test_set_images_batch_argument_validation_without_gpu(lib):
    two = handles(0x1000, 0x2000)
    img = (C.c_uint8 * 100)()
    ptrs = (C.c_void_p * 4)(*[C.addressof(img)] * 4)
    sizes = (C.c_int32 * 6)(10, 10, 10, 10, 10, 10)

    def call(ctxs=two, n=2, imgs=ptrs, n_cams=2, sz=sizes):
        return lib.velo_set_images_batch(C.cast(ctxs, C.c_void_p) if ctxs is not None else None, n,
                                         C.cast(imgs, C.c_void_p) if imgs is not None else None, n_cams,
                                         C.cast(sz, C.c_void_p) if sz is not None else None)
    check_context_list(lib, lambda c, n: call(ctxs=c, n=n))
    assert call(n_cams=0) == -1 and b"0 cameras" in lib.velo_last_error()
    assert call(n_cams=9) == -1 and b"9 cameras" in lib.velo_last_error()
    assert call(imgs=None) == -1 and b"null image list" in lib.velo_last_error()
    assert call(sz=None) == -1 and b"null sizes" in lib.velo_last_error()
    holes = (C.c_void_p * 4)(C.addressof(img), C.addressof(img), C.addressof(img), None)
    assert call(imgs=holes) == -1 and b"context 1: image 1 is null" in lib.velo_last_error()
    assert call(sz=(C.c_int32 * 6)(10, 10, 10, 0, 10, 10)) == -1 and b"context 1: image size 0 x 10" in lib.velo_last_error()
    assert call(sz=(C.c_int32 * 6)(10, 20000, 10, 10, 10, 10)) == -1 and b"context 0: image size" in lib.velo_last_error()
    assert call(sz=(C.c_int32 * 6)(10, 10, 10, 10, 10, 9)) == -1 and b"context 1: row stride 9 < width 10" in lib.velo_last_error()


def test_track_features_batch_argument_validation_without_gpu(lib):
    two = handles(0x1000, 0x2000)
    job = (api.VeloTrackJob * 2)()
    jctx = (C.c_int32 * 2)(0, 1)
    buf = (C.c_float * 64)()
    pts = (C.c_float * 8)()
    for j in range(2):
        job[j].prev_cam, job[j].cam, job[j].prev_xy, job[j].n = 0, 0, C.addressof(pts), 2
    ok = api.lk_params()

    def call(p=ok, ctxs=two, n=2, jc=jctx, jobs=job, nj=2, a=buf, b=buf, c=buf):
        return lib.velo_track_features_batch(C.cast(ctxs, C.c_void_p) if ctxs is not None else None, n,
                                             C.cast(jc, C.c_void_p) if jc is not None else None,
                                             C.cast(jobs, C.c_void_p) if jobs is not None else None, nj,
                                             C.byref(p) if p is not None else None, a, b, c)
    check_context_list(lib, lambda c, n: call(ctxs=c, n=n))
    assert call(nj=-1) == -1 and b"negative job count" in lib.velo_last_error()
    assert call(p=None) == -1 and b"null params" in lib.velo_last_error()
    for bad in (dict(window=4), dict(window=3), dict(window=33), dict(max_level=8), dict(max_level=-1), dict(max_count=101),
                dict(epsilon=-1.0), dict(epsilon=float("nan")), dict(min_eig_threshold=float("inf")), dict(flow_outlier=float("nan"))):
        assert call(p=api.lk_params(**bad)) == -1, bad
    assert call(nj=0, jobs=None, jc=None, a=None, b=None, c=None) == 0       # nothing to do, nothing touched
    assert call(jobs=None) == -1 and b"null jobs" in lib.velo_last_error()
    assert call(jc=None) == -1 and b"null job_ctx" in lib.velo_last_error()
    assert call(jc=(C.c_int32 * 2)(0, 2)) == -1 and b"job 1: context index 2" in lib.velo_last_error()
    assert call(jc=(C.c_int32 * 2)(-1, 0)) == -1 and b"job 0: context index -1" in lib.velo_last_error()
    job[1].n = -4
    assert call() == -1 and b"job 1: negative point count" in lib.velo_last_error()
    job[1].n, job[1].prev_xy = 3, None
    assert call() == -1 and b"job 1: null points" in lib.velo_last_error()
    job[1].n, job[1].prev_xy = 2, C.addressof(pts)
    assert call(a=None) == -1 and b"null next_xy" in lib.velo_last_error()
    assert call(c=None) == -1 and b"null next_xy / status / kept" in lib.velo_last_error()


def test_detect_features_batch_argument_validation_without_gpu(lib):
    two = handles(0x1000, 0x2000)
    job = (api.VeloDetectJob * 2)()
    jctx = (C.c_int32 * 2)(1, 0)
    cnt = (C.c_int32 * 6)()
    xy, resp, fr = (C.c_float * 16)(), (C.c_float * 8)(), (C.c_uint8 * 8)()
    ok = api.gftt_params()

    def call(p=ok, ctxs=two, n=2, jc=jctx, jobs=job, nj=2, cap=4, a=xy, b=resp, c=fr, d=cnt):
        return lib.velo_detect_features_batch(C.cast(ctxs, C.c_void_p) if ctxs is not None else None, n,
                                              C.cast(jc, C.c_void_p) if jc is not None else None,
                                              C.cast(jobs, C.c_void_p) if jobs is not None else None, nj,
                                              C.byref(p) if p is not None else None, cap, a, b, c, d)
    check_context_list(lib, lambda c, n: call(ctxs=c, n=n))
    assert call(p=None) == -1 and b"null params" in lib.velo_last_error()
    assert call(nj=-1) == -1 and b"negative job count" in lib.velo_last_error()
    for bs in (1, 5, 7, 0):
        assert call(p=api.gftt_params(block_size=bs)) == -1 and b"block_size" in lib.velo_last_error()
    for md in (0.0, 0.99, 64.5, -3.0, float("nan"), float("inf")):
        assert call(p=api.gftt_params(min_distance=md)) == -1 and b"min_distance" in lib.velo_last_error(), md
    for q in (0.0, -0.1, 1.0001, float("nan")):
        assert call(p=api.gftt_params(quality_level=q)) == -1 and b"quality_level" in lib.velo_last_error(), q
    assert call(cap=-1) == -1 and b"capacity" in lib.velo_last_error()
    assert call(nj=0) == 0                          # no job: nothing to do, nothing touched
    assert call(jobs=None) == -1 and b"null jobs" in lib.velo_last_error()
    assert call(jc=None) == -1 and b"null job_ctx" in lib.velo_last_error()
    assert call(jc=(C.c_int32 * 2)(0, 5)) == -1 and b"job 1: context index 5" in lib.velo_last_error()
    assert call(d=None) == -1 and b"null counts" in lib.velo_last_error()
    assert call(a=None) == -1 and b"null xy" in lib.velo_last_error()
    job[1].cam, job[1].n_existing = 0, -2
    assert call() == -1 and b"job 1: negative point count" in lib.velo_last_error()
    job[1].n_existing = 5
    assert call() == -1 and b"job 1: null points" in lib.velo_last_error()
    job[1].n_existing, job[1].cam = 0, 8
    assert call() == -1 and b"camera 8" in lib.velo_last_error()
    job[1].cam = -1
    assert call() == -1 and b"camera -1" in lib.velo_last_error()


class _Fake:
    """stands in for a Context where the wrapper must refuse before it calls the library"""
    handle = C.c_void_p(0x1000)

    def __init__(self, lib):
        self._lib = lib


def test_python_wrappers_refuse_unknown_parameters_and_malformed_input(lib):
    ctxs = [_Fake(lib), _Fake(lib)]
    pts = np.zeros((3, 2), np.float32)
    with pytest.raises(TypeError):
        api.track_features_batch(ctxs, [(0, 0, 0, pts)], pyramid_levels=3)
    with pytest.raises(TypeError):
        api.detect_features_batch(ctxs, [(0, 0, None)], use_harris=True)
    with pytest.raises(ValueError):
        api.set_images_batch(ctxs, [[np.zeros((4, 4), np.uint8)]])                                       # one list per context
    with pytest.raises(ValueError):
        api.set_images_batch(ctxs, [[np.zeros((4, 4), np.uint8)], [np.zeros((4, 4), np.uint8)] * 2])   # cameras differ
    with pytest.raises(ValueError):
        api.set_images_batch(ctxs, [[np.zeros((4, 4), np.uint8), np.zeros((4, 5), np.uint8)]] * 2)     # shapes differ inside a context
    with pytest.raises(ValueError):
        api.set_images_batch([], [])
    with pytest.raises(api.VeloError, match="same context"):                                             # the library's own refusal surfaces
        api.track_features_batch([ctxs[0], ctxs[0]], [(0, 0, 0, pts)])


def test_cxx_batch_adaptors_compile_as_cxx11(tmp_path):
    assert os.path.exists(compile_frontend_batch_driver(tmp_path))
