"""The device-resident scan map (velo_map_*) without a GPU: the restatement the GPU tests are measured against (tests/scan_map_ref.py)
against a second form and hand-built cases, its eviction rule, the argument validation of every new entry point, and the header-only
C++ wrapper compiled as C++11."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import scan_map_ref as R
import velo_amd  # noqa: F401
from velo_amd import api, build, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return api.load_library()


def rot(axis, a):
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    T = np.eye(4)
    T[i, i], T[i, j], T[j, i], T[j, j] = c, -s, s, c
    return T


def test_restatement_equals_the_matrix_form_up_to_double_rounding():
    """Second form: xyz.astype(f64) @ M[:3, :3].T + M[:3, 3].  Both sum the same four terms in double; BLAS may order or fuse them
    differently, so the doubles differ by a few units of 2^-53 of the terms' magnitude S, and the floats differ only where a float
    rounding boundary (spaced 2^-24 |q| apart) falls between the two doubles: a share of about 6 * 2^-29 * S / |q| ~ 1e-8 .. 1e-6 of the
    floats for S / |q| up to 100.  Bound: 1e-5, and every differing float differs by one unit in the last place.
    Measured here (1,179,648 floats, 16 poses x 24,576 points): 0 differ."""
    rng = np.random.default_rng(11)
    differ = total = 0
    for k in range(16):
        xyz = (rng.normal(size=(24576, 3)) * [30.0, 3.0, 30.0]).astype(np.float32)
        pose = rot(k % 3, rng.uniform(-3, 3)) @ rot((k + 1) % 3, rng.uniform(-0.2, 0.2))
        pose[:3, 3] = rng.normal(size=3) * [50.0, 1.0, 50.0]
        ref = rot(1, rng.uniform(-3, 3))
        ref[:3, 3] = rng.normal(size=3) * 40.0
        ref_inv = np.linalg.inv(ref)
        M = R.compose(ref_inv, pose)
        a = R.move(xyz, M)
        b = (xyz.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)
        ne = a.view(np.uint32) != b.view(np.uint32)
        differ += int(ne.sum())
        total += a.size
        if ne.any():
            step = np.abs(a.view(np.int32)[ne].astype(np.int64) - b.view(np.int32)[ne].astype(np.int64))
            assert step.max() == 1
        # the composed matrix against numpy's product: double rounding of four terms
        np.testing.assert_allclose(M, (ref_inv @ pose)[:3], rtol=0, atol=8 * np.finfo(np.float64).eps * (np.abs(ref_inv) @ np.abs(pose))[:3].max())
    print(f"restatement vs matrix form: {differ} of {total} floats differ")
    assert differ <= 1e-5 * total


def test_hand_built_matrices_are_exact():
    xyz = np.array([[1.0, 2.0, 3.0], [-4.5, 0.25, 8.0], [0.0, 0.0, 0.0], [1024.0, -0.5, 3.0e-3]], dtype=np.float32)
    eye = np.eye(4)
    got = R.move(xyz, R.compose(eye, eye))
    assert got.tobytes() == xyz.tobytes()
    turn = np.array([[0.0, -1.0, 0.0, 0.0], [1.0, 0.0, 0.0, 0.0], [0.0, 0.0, 1.0, 0.0], [0.0, 0.0, 0.0, 1.0]])     # 90 degrees about z
    want = np.stack([-xyz[:, 1], xyz[:, 0], xyz[:, 2]], axis=1) + np.float32(0.0)                                   # (-0.0 + 0.0 = +0.0)
    assert R.move(xyz, R.compose(eye, turn)).tobytes() == want.astype(np.float32).tobytes()
    assert R.move(xyz, R.compose(turn, eye)).tobytes() == want.astype(np.float32).tobytes()
    shift = np.eye(4)
    shift[:3, 3] = [1000.0, -2.0, 0.5]
    want = (xyz.astype(np.float64) + shift[:3, 3]).astype(np.float32)
    assert R.move(xyz, R.compose(eye, shift)).tobytes() == want.tobytes()
    # the translation and its inverse compose to the identity exactly
    back = np.eye(4)
    back[:3, 3] = -shift[:3, 3]
    assert np.array_equal(R.compose(back, shift), eye[:3])


def test_negative_zero_goes_in_and_positive_zero_comes_out():
    xyz = np.array([[-0.0, -0.0, -0.0], [-0.0, 1.0, -0.0]], dtype=np.float32)
    assert np.signbit(xyz[0]).all()
    got = R.move(xyz, R.compose(np.eye(4), np.eye(4)))
    assert not np.signbit(got).any()
    assert got.tobytes() == np.array([[0.0, 0.0, 0.0], [0.0, 1.0, 0.0]], dtype=np.float32).tobytes()


def scan(n, rings, seed):
    rng = np.random.default_rng(seed)
    off = np.linspace(0, n, rings + 1).astype(np.int32)
    return rng.normal(size=(n, 3)).astype(np.float32), off


def test_eviction_order_under_both_limits():
    m = R.ScanMapRef(3, 1000)
    for f in range(6):
        xyz, off = scan(100, 4, f)
        assert m.insert(f, xyz, off, np.eye(4)) == (0 if f < 3 else 1)
        assert m.frames() == list(range(max(0, f - 2), f + 1))
    assert m.info()["evictions"] == 3 and m.points == 300
    # the point budget: 250 + 250 + 250 in, then a scan of 600 evicts two at once (750 + 600 > 1000, 500 + 600 > 1000, 250 + 600 fits)
    m = R.ScanMapRef(10, 1000)
    for f in range(3):
        assert m.insert(f, *scan(250, 5, f), np.eye(4)) == 0
    assert m.insert(3, *scan(600, 5, 3), np.eye(4)) == 2
    assert m.frames() == [2, 3] and m.points == 850 and m.evictions == 2
    # a frame that is present is refused
    assert m.insert(3, *scan(10, 1, 9), np.eye(4)) is None and m.frames() == [2, 3]


def test_oversized_scan_is_refused_and_the_window_stays():
    m = R.ScanMapRef(4, 500)
    for f in range(2):
        m.insert(f, *scan(200, 2, f), np.eye(4))
    before = [(s[0], s[1].tobytes(), s[2].tobytes()) for s in m.scans]
    assert m.insert(7, *scan(501, 2, 7), np.eye(4)) is None
    assert m.insert(8, np.zeros((0, 3), np.float32), np.zeros(1, np.int32), np.eye(4)) is None
    assert [(s[0], s[1].tobytes(), s[2].tobytes()) for s in m.scans] == before and m.evictions == 0
    assert m.insert(9, *scan(500, 2, 9), np.eye(4)) == 2 and m.frames() == [9]


def test_empty_rings_are_dropped():
    xyz = np.arange(15, dtype=np.float32).reshape(5, 3)
    m = R.ScanMapRef(4, 100)
    m.insert(0, xyz, [0, 0, 2, 2, 2, 5, 5], np.eye(4))
    m.insert(1, xyz, [0, 1, 5], np.eye(4))
    assert m.scans[0][2].tolist() == [0, 2, 5] and m.info()["rings"] == 4
    cloud, off = m.materialise(np.eye(4))
    assert off.tolist() == [0, 2, 5, 6, 10] and cloud.tobytes() == np.concatenate([xyz, xyz]).tobytes()


def test_materialise_of_a_small_drive_equals_scan_to_map_construction():
    """the construction of synth.scan_to_map (every scan moved into the newest pose's frame), to float rounding"""
    d = synth.drive(3, n_beams=8, n_azimuth=64)
    Cm = synth.VELO_TO_CAM.astype(np.float64)
    poses = [Cm @ P @ np.linalg.inv(Cm) for P in d["poses_velo"]]
    m = R.ScanMapRef(8, 1 << 20)
    for k, (xyz, off) in enumerate(d["frames"]):
        m.insert(k, xyz, off, poses[k])
    cloud, off = m.materialise(np.linalg.inv(poses[-1]))
    want = np.concatenate([xyz.astype(np.float64) @ (np.linalg.inv(poses[-1]) @ poses[k])[:3, :3].T + (np.linalg.inv(poses[-1]) @ poses[k])[:3, 3]
                           for k, (xyz, _) in enumerate(d["frames"])])
    np.testing.assert_allclose(cloud, want, rtol=0, atol=2.0 ** -23 * np.abs(want).max())
    assert off[-1] == len(cloud) and (np.diff(off) > 0).all()


@pytest.mark.skipif(os.path.exists("/dev/kfd"), reason="this check is for boxes without a GPU")
def test_map_create_without_a_device_fails_loudly(lib):
    h = C.c_void_p()
    assert lib.velo_map_create(C.byref(h), 0, 17, 1 << 21) == -5 and not h.value          # VELO_ERR_NODEVICE, as velo_cache_create
    with pytest.raises(api.VeloError):
        api.ScanMap(0)


def test_argument_validation_without_a_device(lib):
    h = C.c_void_p()
    pose = (C.c_double * 16)(*np.eye(4).reshape(-1))
    assert lib.velo_map_create(None, 0, 17, 100) == -1
    assert lib.velo_map_create(C.byref(h), 0, 0, 100) == -1 and lib.velo_map_create(C.byref(h), 0, -3, 100) == -1      # max_scans < 1
    assert lib.velo_map_create(C.byref(h), 0, 17, 0) == -1 and lib.velo_map_create(C.byref(h), 0, 17, (1 << 30) + 1) == -1
    assert not h.value
    assert lib.velo_map_destroy(None) == 0
    fake = C.c_void_p(0x1000)
    n = C.c_int32(7)
    assert lib.velo_map_insert(None, fake, 0, 0, pose, C.byref(n)) == -1 and n.value == 0
    assert lib.velo_map_insert(fake, None, 0, 0, pose, None) == -1
    assert lib.velo_map_set_pose(None, 0, pose) == -1
    assert lib.velo_map_drop(None, 0) == -1
    assert lib.velo_map_clear(None) == -1
    assert lib.velo_map_frames(None, None, 0) == 0
    info = (C.c_int64 * 8)()
    assert lib.velo_map_info(None, info) == -1 and lib.velo_map_info(fake, None) == -1
    assert lib.velo_map_get_scan(None, 0, None, 0, C.byref(n), None, 0, None, None) == -1 and n.value == 0
    assert lib.velo_map_load(None, fake, pose) == -1 and lib.velo_map_load(fake, None, pose) == -1
    assert lib.velo_map_load_batch(None, None, 1, pose) == -1
    maps = (C.c_void_p * 2)(fake, fake)
    ctxs = (C.c_void_p * 2)(fake, fake)
    poses = (C.c_double * 32)()
    assert lib.velo_map_load_batch(maps, ctxs, 2, poses) == -1 and b"same context" in lib.velo_last_error()
    assert lib.velo_map_load_batch(maps, ctxs, 0, poses) == -1
    ctxs = (C.c_void_p * 2)(fake, None)
    assert lib.velo_map_load_batch(maps, ctxs, 2, poses) == -1 and b"null" in lib.velo_last_error()


def test_signatures_cover_the_new_section():
    names = [n for n in api.SIGNATURES if n.startswith("velo_map_")]
    assert sorted(names) == sorted(f"velo_map_{s}" for s in ("create", "destroy", "insert", "set_pose", "drop", "clear", "frames", "info",
                                                              "get_scan", "load", "load_batch"))
    for name in ("insert", "set_pose", "drop", "clear", "frames", "info", "get_scan", "load"):
        assert callable(getattr(api.ScanMap, name))
    assert callable(api.map_load_batch)


def compile_driver(tmp_path) -> str:
    build.build_hip()
    exe = str(tmp_path / "test_scan_map")
    csrc = os.path.dirname(build.LIB)
    subprocess.run(["g++", "-std=c++11", "-pedantic", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                    os.path.join(CPP, "test_scan_map.cpp"), "-o", exe, "-L", csrc, "-lvelo_hip", f"-Wl,-rpath,{csrc}",
                    "-Wl,-rpath,/opt/rocm/lib"], check=True)
    return exe


def test_wrapper_compiles_as_cxx11_and_links(tmp_path):
    out = subprocess.run([compile_driver(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 0 and "scan map wrapper linked" in out.stdout
