"""CPU checks of velo_frames_put_frame[_batch] (a frame put with its keypoint depth computed on the device): the arguments that are
refused before any context is read (no GPU needed), the ctypes mirror of velo_frame_cam against the header, and -- on the ORACLE's
output -- the input conditions tests/test_gpu_frame_depth.py relies on: its cases hold keypoints with and without depth."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import velo_amd  # noqa: F401
from velo_amd import api, build, synth
from test_depth_oracle import crafted_rings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "depth_mini.npz")


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return api.load_library()


def test_argument_validation_without_gpu(lib):
    fake = C.c_void_p(0x1000)                       # never dereferenced: these checks come before any context is read
    cams = (api.VeloFrameCam * 8)()
    n_wd = (C.c_int32 * 8)()
    table = C.cast(cams, C.c_void_p)
    assert lib.velo_frames_put_frame(None, 0, 0, table, 0.015, 0, n_wd) == -1 and b"null ctx" in lib.velo_last_error()
    assert lib.velo_frames_put_frame(fake, 0, 0, None, 0.015, 0, n_wd) == -1 and b"null cams" in lib.velo_last_error()
    for frame in (-1, 1 << 22):
        assert lib.velo_frames_put_frame(fake, frame, 0, table, 0.015, 0, n_wd) == -1 and b"frame" in lib.velo_last_error()
    for flags in (2, 3, -1):
        assert lib.velo_frames_put_frame(fake, 0, 0, table, 0.015, flags, n_wd) == -1 and b"unknown flags" in lib.velo_last_error()
    frames, side = (C.c_int32 * 2)(0, 0), (C.c_int32 * 2)(0, 0)
    arr = (C.c_void_p * 2)(fake, fake)
    batch = lambda a, n, f=frames, t=side, k=table: lib.velo_frames_put_frame_batch(a, n, f, t, k, 0.015, 0, None)   # noqa: E731
    assert batch(arr, 2) == -1 and b"same context" in lib.velo_last_error()
    assert batch((C.c_void_p * 2)(fake, None), 2) == -1 and b"null" in lib.velo_last_error()
    assert batch(None, 1) == -1 and b"null context list" in lib.velo_last_error()
    assert batch(arr, 0) == -1 and batch(arr, -3) == -1
    assert batch(arr, 1, f=None) == -1 and b"null frames" in lib.velo_last_error()
    assert batch(arr, 1, t=None) == -1 and b"null frames / of_target" in lib.velo_last_error()
    assert batch(arr, 1, k=None) == -1 and b"null cams" in lib.velo_last_error()


def test_frame_cam_mirror_has_the_headers_layout(tmp_path):
    src = r'''
#include <stdio.h>
#include <stddef.h>
#include "velo_hip.h"
int main(void) {
  printf("%zu %zu %zu %zu %zu %zu %d\n", sizeof(velo_frame_cam), offsetof(velo_frame_cam, ids), offsetof(velo_frame_cam, keypoints_xy),
         offsetof(velo_frame_cam, rows), offsetof(velo_frame_cam, n), offsetof(velo_frame_cam, bounds), VELO_PUT_OBSERVE);
  return 0; }
'''
    cfile, exe = str(tmp_path / "probe.c"), str(tmp_path / "probe")
    open(cfile, "w").write(src)
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe], check=True)
    got = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    K = api.VeloFrameCam
    assert got == [C.sizeof(K), K.ids.offset, K.keypoints_xy.offset, K.rows.offset, K.n.offset, K.bounds.offset, api.VELO_PUT_OBSERVE]


def test_frame_cam_wrapper_checks_shapes():
    w = synth.cam_window()
    with pytest.raises(ValueError):
        api.FrameCam([1, 2, 3], np.zeros((2, 2)), w)
    with pytest.raises(ValueError):
        api.FrameCam([1, 2], np.zeros((2, 2)), w, rows=np.zeros((3, 64), np.uint8))
    with pytest.raises(ValueError):
        api.FrameCam([1, 2], np.zeros((2, 2)), w[:3])
    k = api.FrameCam([], np.zeros((0, 2)), w, rows=np.zeros((0, 64), np.uint8)).as_struct()
    assert k.n == 0 and k.ids is None and k.rows is not None             # an empty row set is still a row set
    assert api.FrameCam([4], [[0.1, 0.2]], w).as_struct().rows is None
    assert list(api.FrameCam([4], [[0.1, 0.2]], w).as_struct().bounds) == list(w)


# ---- what the GPU tests rely on, shown on the oracle: both kinds of keypoint occur ---------------------------------------------------
@pytest.mark.parametrize("cam", [0, 1])
@pytest.mark.parametrize("n_rings", [150, 65, 64])
def test_crafted_rings_hold_keypoints_with_and_without_depth(cam, n_rings):
    xyz, off = crafted_rings(n_rings=n_rings)
    proj = O.project_lidar(xyz, off, synth.CAM_TRANS[cam], synth.cam_window())
    _, has = O.depth_association(*proj, synth.keypoints_in_window(700, seed=3), 0.2)
    assert (has >= 0).sum() >= 50 and (has == -1).sum() >= 50


def test_the_wide_threshold_case_and_the_small_scan_give_depth():
    xyz, off = crafted_rings(n_rings=150)
    proj = O.project_lidar(xyz, off, synth.CAM_TRANS[0], synth.cam_window())
    kps = synth.keypoints_in_window(520, seed=10)
    tight, wide = [(O.depth_association(*proj, kps, t)[1] >= 0).sum() for t in (0.2, 1e9)]
    assert wide > tight > 0 and wide > 520 // 2          # every keypoint two neighbouring rings bracket, whatever the gap
    d = synth.scan_pair(16, 128)
    w = np.float64([-2.0, 2.0, -1.0, 1.0])
    for side in ("tgt", "src"):
        proj = O.project_lidar(d[side + "_xyz"], d[side + "_off"], synth.CAM_TRANS[1], w)
        assert (O.depth_association(*proj, synth.keypoints_in_window(400, seed=12, window=w), 0.3)[1] >= 0).sum() > 50


def test_depth_mini_holds_both_kinds():
    g = np.load(GOLDEN)
    assert (g["has_depth"] >= 0).any() and (g["has_depth"] == -1).any()
    proj = O.project_lidar(g["xyz"], g["off"], g["cam_t"], g["window"])
    _, has = O.depth_association(*proj, g["keypoints"], float(g["thresh"]))
    assert np.array_equal(has, g["has_depth"])
