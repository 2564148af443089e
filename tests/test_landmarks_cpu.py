"""CPU checks of the resident landmark store's boundary: tests/landmarks_ref.py (the Python transcription of main.cpp:614-679 and
getLandmarksAtFrame) against hand-built cases, and the argument validation of the velo_landmarks_* entries, which refuses bad
arguments with the library's usual argument error before any context is touched (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest

import landmarks_ref as LR
import velo_amd  # noqa: F401
from velo_amd import api, build


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return api.load_library()


def hand_book():
    """2 cameras, 3 frames.  id 0: 2-D in (f0,c0), (f0,c1), (f2,c0) and 3-D in (f1,c1); id 2: 2-D once; id 4: 3-D in (f1,c0), (f2,c0), (f2,c1)."""
    b = LR.LandmarkBook(2)
    kp = lambda *v: np.array(v, dtype=np.float32).reshape(-1, 2)      # noqa: E731
    cl = lambda *v: np.array(v, dtype=np.float32).reshape(-1, 3)      # noqa: E731
    b.observe_frame(0, [kp(.1, .2, .5, .5), kp(.11, .2)], [[0, 2], [0]], [[-1, -1], [-1]], [cl(), cl()])
    b.observe_frame(1, [kp(.3, .3), kp(.12, .2)], [[4], [0]], [[0], [0]], [cl(1, 2, 3), cl(4, 5, 6)])
    b.observe_frame(2, [kp(.31, .3, .13, .2), kp(.32, .3)], [[4, 0], [4]], [[1, -1], [0]], [cl(9, 9, 9, 1.1, 2.1, 3.1), cl(1.2, 2.2, 3.2)])
    return b


def test_reference_bookkeeping_on_a_hand_built_case():
    b = hand_book()
    assert b.keypoint_obs_count == [4, 0, 1, 0, 3]
    assert len(b.keypoint_added) == 5 and not any(b.keypoint_added)
    assert b.ids_to_triangulate(0) == [0]                  # id 2 has one observation
    assert b.ids_to_triangulate(1) == [0, 4] and b.ids_to_triangulate(2) == [0, 4]
    obs, off, p0, init = b.csr([0, 4])
    assert off.tolist() == [0, 4, 7] and init.tolist() == [0, 0] and not p0.any()
    # id 0: its 3-D observation first, then 2-D camera-major and frame-ascending; id 4: 3-D camera-major, frame-ascending
    assert [(int(o["kind"]), int(o["frame"]), int(o["cam"])) for o in obs] == [(0, 1, 1), (1, 0, 0), (1, 2, 0), (1, 0, 1), (0, 1, 0), (0, 2, 0), (0, 2, 1)]
    assert obs["s"][0].tolist() == [4, 5, 6] and obs["s"][2].tolist() == [np.float32(.13), np.float32(.2), 0]
    assert obs["s"][5].tolist() == [np.float32(1.1), np.float32(2.1), np.float32(3.1)]       # has_depth 1 -> the cloud's second point
    b.store([0, 4], np.array([[1, 2, 4], [2, 4, 8]], dtype=np.float32))
    assert b.keypoint_added == [True, False, False, False, True]
    _, _, p0, init = b.csr([0, 4])
    assert init.tolist() == [1, 1] and p0.tolist() == [[1, 2, 4], [2, 4, 8]]


def test_reference_landmarks_at_frame_on_a_hand_built_case():
    b = hand_book()
    b.store([4], np.array([[2, 4, 8]], dtype=np.float32))
    M = np.eye(4)
    M[:3, 3] = [1, -1, .5]
    M[3, 3] = 2.0
    ids, xyz = b.landmarks_at_frame(M, 2)                   # ids 4 and 0 are seen, only 4 is added
    assert ids.tolist() == [4] and xyz.tolist() == [[1.5, 1.5, 4.25]]
    ids, xyz = b.landmarks_at_frame(M, 0)
    assert ids.tolist() == [] and xyz.shape == (0, 3)
    b.store([0], np.array([[1, 1, 1]], dtype=np.float32))
    ids, _ = b.landmarks_at_frame(M, 2)
    assert ids.tolist() == [0, 4]                           # the std::map's order, not camera 0's


def test_main_sequence_has_the_cases_the_gpu_test_relies_on():
    seq = LR.main_sequence()
    b = LR.LandmarkBook(2)
    seen_counts = {5: set(), 70000: set()}
    both = False
    for f, per_cam in enumerate(seq["frames"]):
        b.observe_frame(f, [c[1] for c in per_cam], [c[0] for c in per_cam], [c[2] for c in per_cam], [c[3] for c in per_cam])
        both = both or bool(set(per_cam[0][0].tolist()) & set(per_cam[1][0].tolist()) - {5})
        for id in seen_counts:
            seen_counts[id].add(b.keypoint_obs_count[id])
    assert {64, 130} <= seen_counts[5] and {64, 65} <= seen_counts[70000]
    assert [b.keypoint_obs_count[i] for i in (50, 51, 52, 53)] == [0, 1, 2, 3] and both
    assert all(len(c[0]) == 0 for c in seq["frames"][60])
    kinds = {id: ({0} if any(b.keypoint_obs3[id][c] for c in range(2)) else set()) | ({1} if any(b.keypoint_obs2[id][c] for c in range(2)) else set())
             for id in range(100, 300) if b.keypoint_obs_count[id] >= 3}
    assert {frozenset(v) for v in kinds.values()} == {frozenset({0}), frozenset({1}), frozenset({0, 1})}
    skips = [id for id in range(100, 300) for fr in [sorted(set(b.keypoint_obs2[id][0]) | set(b.keypoint_obs3[id][0]) | set(b.keypoint_obs2[id][1]) | set(b.keypoint_obs3[id][1]))]
             if len(fr) >= 2 and fr[-1] - fr[0] + 1 > len(fr)]
    assert len(skips) > 5
    assert sum(len(c[0]) for per_cam in seq["frames"] for c in per_cam) > 400      # far more than the log's starting capacity in the GPU test


def test_argument_validation_without_gpu(lib):
    fake = C.c_void_p(0x1000)                       # never dereferenced: every argument is checked before the context is touched
    ct = (C.c_float * 6)(0, 0, 0, .5, 0, 0)
    err = lib.velo_last_error
    assert lib.velo_landmarks_reset(None, 2, ct, 0) == -1 and b"null ctx" in err()
    for nc in (0, -1, 9):
        assert lib.velo_landmarks_reset(fake, nc, ct, 0) == -1 and b"cameras" in err()
    assert lib.velo_landmarks_reset(fake, 2, None, 0) == -1 and b"null cam_trans" in err()
    assert lib.velo_landmarks_reset(fake, 2, ct, -5) == -1 and b"log capacity" in err()
    bad = (C.c_float * 6)(0, float("nan"), 0, 0, 0, 0)
    assert lib.velo_landmarks_reset(fake, 2, bad, 0) == -1 and b"not finite" in err()

    pose = (C.c_double * 6)()
    assert lib.velo_landmarks_set_pose(None, 0, pose) == -1
    assert lib.velo_landmarks_set_pose(fake, -1, pose) == -1 and b"frame -1" in err()
    assert lib.velo_landmarks_set_pose(fake, 1 << 22, pose) == -1 and b"frame" in err()
    assert lib.velo_landmarks_set_pose(fake, 0, None) == -1 and b"null pose" in err()
    pose[4] = float("inf")
    assert lib.velo_landmarks_set_pose(fake, 0, pose) == -1 and b"not finite" in err()

    def observe(ids, has, n_cloud=2, frame=0, cam=0, ctx=fake, kp=True, cloud=True):
        i = np.asarray(ids, dtype=np.int32)
        h = np.asarray(has, dtype=np.int32)
        k = np.zeros((max(len(i), 1), 2), dtype=np.float32)
        c = np.zeros((max(n_cloud, 1), 3), dtype=np.float32)
        vp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
        return lib.velo_landmarks_observe(ctx, frame, cam, vp(i), vp(k) if kp else None, vp(h), vp(c) if cloud else None, n_cloud, len(i))
    assert observe([1], [-1], ctx=None) == -1 and b"null ctx" in err()
    assert observe([1], [-1], frame=-2) == -1 and b"frame -2" in err()
    assert observe([1], [-1], cam=8) == -1 and b"camera 8" in err()
    assert observe([1], [-1], cam=-1) == -1 and b"camera -1" in err()
    assert observe([1], [-1], kp=False) == -1 and b"null ids / keypoints" in err()
    assert observe([1], [-1], n_cloud=-1) == -1 and b"negative count" in err()
    assert observe([3, -4], [-1, -1]) == -1 and b"negative id -4" in err()
    assert observe([3, 1 << 26], [-1, -1]) == -1 and b"id 67108864" in err()
    assert observe([3, 9, 3], [-1, -1, -1]) == -1 and b"id 3 appears twice" in err()
    assert observe([3, 9], [0, 2]) == -1 and b"has_depth 2 outside the cloud of 2" in err()
    assert observe([3, 9], [0, -2]) == -1 and b"has_depth -2" in err()
    assert observe([3], [0], n_cloud=1, cloud=False) == -1 and b"null cloud" in err()
    assert lib.velo_landmarks_observe(fake, 0, 0, None, None, None, None, 0, -1) == -1 and b"negative count" in err()

    n = C.c_int32(7)
    assert lib.velo_landmarks_triangulate(None, 0, None, None, None, 0, C.byref(n)) == -1 and b"null ctx" in err()
    assert lib.velo_landmarks_triangulate(fake, -1, None, None, None, 0, C.byref(n)) == -1 and b"frame -1" in err()
    assert lib.velo_landmarks_triangulate(fake, 0, None, None, None, -1, C.byref(n)) == -1 and b"negative capacity" in err()
    assert lib.velo_landmarks_triangulate(fake, 0, None, None, None, 4, None) == -1 and b"null n_out" in err()
    fr = np.zeros(2, dtype=np.int32)
    no = np.zeros(2, dtype=np.int32)
    vp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    arr = (C.c_void_p * 2)(fake, fake)
    assert lib.velo_landmarks_triangulate_batch(C.cast(arr, C.c_void_p), 2, vp(fr), None, None, None, 4, vp(no)) == -1 and b"same context" in err()
    arr = (C.c_void_p * 2)(fake, None)
    assert lib.velo_landmarks_triangulate_batch(C.cast(arr, C.c_void_p), 2, vp(fr), None, None, None, 4, vp(no)) == -1 and b"null" in err()
    assert lib.velo_landmarks_triangulate_batch(C.cast(arr, C.c_void_p), 0, vp(fr), None, None, None, 4, vp(no)) == -1 and b"0 contexts" in err()
    arr = (C.c_void_p * 2)(fake, C.c_void_p(0x2000))
    assert lib.velo_landmarks_triangulate_batch(C.cast(arr, C.c_void_p), 2, None, None, None, None, 4, vp(no)) == -1 and b"null frames" in err()

    M = (C.c_double * 16)(*np.eye(4).reshape(-1))
    assert lib.velo_landmarks_at_frame(None, 0, M, None, None, 0, C.byref(n)) == -1
    assert lib.velo_landmarks_at_frame(fake, -3, M, None, None, 0, C.byref(n)) == -1 and b"frame -3" in err()
    assert lib.velo_landmarks_at_frame(fake, 0, None, None, None, 0, C.byref(n)) == -1 and b"null pose_inv" in err()
    assert lib.velo_landmarks_at_frame(fake, 0, M, None, None, 0, None) == -1 and b"null n_out" in err()
    assert lib.velo_landmarks_at_frame(fake, 0, M, None, None, -1, C.byref(n)) == -1 and b"negative capacity" in err()
    M[5] = float("nan")
    assert lib.velo_landmarks_at_frame(fake, 0, M, None, None, 0, C.byref(n)) == -1 and b"not finite" in err()

    ids = np.array([1, -2], dtype=np.int32)
    assert lib.velo_landmarks_get(None, vp(ids), 2, None, None, None) == -1
    assert lib.velo_landmarks_get(fake, vp(ids), -1, None, None, None) == -1 and b"negative count" in err()
    assert lib.velo_landmarks_get(fake, None, 2, None, None, None) == -1 and b"null ids" in err()
    assert lib.velo_landmarks_get(fake, vp(ids), 2, None, None, None) == -1 and b"negative id -2" in err()
    assert lib.velo_landmarks_info(None, None) == -1
