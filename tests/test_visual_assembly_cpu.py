"""CPU checks of the match assembly's boundary: tests/visual_ref.py (matchUsingId, velo.h:627-654 and the landmark rule in Python
containers) against a second, vectorised form and against hand-built cases; the occurrence counts the GPU test relies on; the
struct sizes; and the argument validation of velo_frames_* / velo_build_matches* / velo_get_visual, which refuses bad arguments
with the library's usual argument error before any context is touched (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest

import visual_ref as VR
import velo_amd  # noqa: F401
from velo_amd import api, build


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return api.load_library()


def shared_inputs():
    """every (frame1, frame2, cam_trans, landmarks) the GPU test assembles, with made-up landmark points where it has the device's"""
    out = []
    for sizes in VR_SIZES:
        f1, f2, ct = VR.random_pair(100 + sum(sizes[0]) + 7 * sum(sizes[1]), sizes[0], sizes[1])
        out.append((f1, f2, ct, None))
    out.append(VR.id_cases() + (None,))
    out.append(VR.id_cases() + ({5: np.float32([1, 2, 3]), 9: np.float32([4, 5, 6]), 12: np.float32([7, 8, 9])},))
    seq, fr1, fr2 = VR.landmark_case()
    book = VR.walk_book(seq, fr2)
    Minv = np.linalg.inv(api.pose_vec_to_mat(seq["poses"][fr2]))
    out.append((seq["frames"][fr1], seq["frames"][fr2], seq["cam_trans"], VR.landmarks_dict(book, Minv, fr2)))
    return out


K = VR.CHUNK
VR_SIZES = [((0,), (0,)), ((1,), (1,)), ((5,), (0,)), ((0,), (5,)), ((K - 1,), (K - 1,)), ((K,), (K,)), ((K + 1,), (K + 1,)),
            ((700,), (3 * K + 1,)), ((3 * K + 1, 0), (40, 300)), ((300, 500), (0, 2 * K))]


def test_match_using_id_on_hand_built_cases():
    assert VR.match_using_id([4, 8, 4, 6], [6, 4, 5, 4]) == [(3, 0), (2, 1), (2, 3)]         # last index of 4 wins; 4 twice in frame2
    assert VR.match_using_id([], [1, 2]) == [] and VR.match_using_id([1, 2], []) == []
    f1, f2, ct = VR.id_cases()
    recs, per_cam = VR.assemble(f1, f2, ct)
    pairs = list(zip(recs["point1"].tolist(), recs["point2"].tolist()))
    assert pairs == [(6, 0), (9, 2), (7, 3), (6, 4), (4, 6), (3, 7), (9, 8), (11, 9), (10, 10)] and per_cam.tolist() == [9]
    assert recs["d1"].tolist() == [1, 0, 0, 1, 1, 0, 0, 0, 1] and recs["d2"].tolist() == [1, 1, 0, 1, 1, 0, 1, 0, 1]
    assert recs["p3_1"][1].tolist() == [0, 0, 0] and recs["p3_2"][0].tolist() == f2[0][3][0].tolist()
    assert recs["t_cam"][3].tolist() == ct[0].tolist() and not recs["pad"].any()
    # a landmark replaces frame2's depth point (id 9 at ind2 2) and gives depth where there was none (id 5 at ind2 7)
    lm = {5: np.float32([1, 2, 3]), 9: np.float32([4, 5, 6])}
    recs, _ = VR.assemble(f1, f2, ct, lm)
    assert recs["p3_2"][1].tolist() == [4, 5, 6] and recs["p3_2"][6].tolist() == [4, 5, 6] and recs["p3_2"][5].tolist() == [1, 2, 3]
    assert recs["d2"].tolist() == [1, 1, 0, 1, 1, 1, 1, 0, 1]


def test_restatement_equals_the_vectorised_form():
    n_records = 0
    for f1, f2, ct, lm in shared_inputs():
        a, na = VR.assemble(f1, f2, ct, lm)
        b, nb = VR.assemble_vectorised(f1, f2, ct, lm)
        assert na.tolist() == nb.tolist()
        assert a.tobytes() == b.tobytes()
        n_records += len(a)
    assert n_records > 1500                 # the inputs are not degenerate


def test_inputs_hold_the_cases_the_gpu_test_relies_on():
    seq, fr1, fr2 = VR.landmark_case()
    book = VR.walk_book(seq, fr2)
    lm = VR.landmarks_dict(book, np.eye(4), fr2)
    per_cam = VR.occurrence_counts(seq["frames"][fr1], seq["frames"][fr2], lm)
    assert len(per_cam) == 2
    for combos, replaced, fresh in per_cam:
        assert all(v >= 5 for v in combos.values()), combos
        assert replaced >= 5 and fresh >= 5, (replaced, fresh)
    assert all(len(c[0]) <= 1100 for f in (fr1, fr2) for c in seq["frames"][f])
    # added and not-added ids are mixed among the matched ones
    ids2 = np.concatenate([c[0] for c in seq["frames"][fr2]])
    assert 20 < sum(int(i) in lm for i in ids2) < len(ids2) - 20
    # the random pairs share ids, and the sizes straddle the compaction's chunk
    for sizes in VR_SIZES:
        f1, f2, ct = VR.random_pair(1, sizes[0], sizes[1])
        _, n = VR.assemble(f1, f2, ct)
        for cam in range(len(n)):
            small = min(sizes[0][cam], sizes[1][cam])
            assert n[cam] <= small and (small < 5 or n[cam] >= small // 2)


def test_struct_sizes(lib):
    assert api.MATCH_DTYPE.itemsize == 68 and api.MATCH_DTYPE.fields["cam"][1] == 52 and api.MATCH_DTYPE.fields["pad"][1] == 66
    for name in ("velo_frames_reset", "velo_frames_put", "velo_frames_drop", "velo_frames_info", "velo_frames_count", "velo_build_matches",
                 "velo_build_matches_batch", "velo_get_visual"):
        assert hasattr(lib, name) and name in api.SIGNATURES


def test_argument_validation_without_gpu(lib):
    fake = C.c_void_p(0x1000)                       # never dereferenced: every argument is checked before the context is touched
    ct = (C.c_float * 6)(0, 0, 0, .5, 0, 0)
    err = lib.velo_last_error
    assert lib.velo_frames_reset(None, 2, ct, 0) == -1 and b"null ctx" in err()
    for nc in (0, -1, 9):
        assert lib.velo_frames_reset(fake, nc, ct, 0) == -1 and b"cameras" in err()
    assert lib.velo_frames_reset(fake, 2, None, 0) == -1 and b"null cam_trans" in err()
    assert lib.velo_frames_reset(fake, 2, ct, -5) == -1 and b"arena capacity" in err()
    bad = (C.c_float * 6)(0, float("nan"), 0, 0, 0, 0)
    assert lib.velo_frames_reset(fake, 2, bad, 0) == -1 and b"not finite" in err()

    def put(ids, has, n_cloud=2, frame=0, cam=0, ctx=fake, kp=True, cloud=True):
        i = np.asarray(ids, dtype=np.int32)
        h = np.asarray(has, dtype=np.int32)
        k = np.zeros((max(len(i), 1), 2), dtype=np.float32)
        c = np.zeros((max(n_cloud, 1), 3), dtype=np.float32)
        vp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
        return lib.velo_frames_put(ctx, frame, cam, vp(i), vp(k) if kp else None, vp(h), vp(c) if cloud else None, n_cloud, len(i))
    assert put([1], [-1], ctx=None) == -1 and b"null ctx" in err()
    assert put([1], [-1], frame=-2) == -1 and b"frame -2" in err()
    assert put([1], [-1], frame=1 << 22) == -1 and b"frame" in err()
    assert put([1], [-1], cam=8) == -1 and b"camera 8" in err()
    assert put([1], [-1], cam=-1) == -1 and b"camera -1" in err()
    assert put([1], [-1], kp=False) == -1 and b"null ids / keypoints" in err()
    assert put([1], [-1], n_cloud=-1) == -1 and b"negative count" in err()
    assert put([3, -4], [-1, -1]) == -1 and b"negative id -4" in err()
    assert put([3, 1 << 26], [-1, -1]) == -1 and b"id 67108864" in err()
    assert put([3, 9], [0, 2]) == -1 and b"has_depth 2 outside the cloud of 2" in err()
    assert put([3, 9], [0, -2]) == -1 and b"has_depth -2" in err()
    assert put([3], [0], n_cloud=1, cloud=False) == -1 and b"null pointer" in err()
    assert lib.velo_frames_put(fake, 0, 0, None, None, None, None, 0, -1) == -1 and b"negative count" in err()

    assert lib.velo_frames_drop(None, 0) == -1 and b"null ctx" in err()
    assert lib.velo_frames_drop(fake, -1) == -1 and b"frame -1" in err()
    assert lib.velo_frames_info(None, None) == -1 and lib.velo_frames_info(fake, None) == -1
    assert lib.velo_frames_count(None, 0, None, None) == -1 and b"null ctx" in err()
    assert lib.velo_frames_count(fake, -1, None, None) == -1 and b"frame -1" in err()
    assert lib.velo_frames_count(fake, 1 << 22, None, None) == -1 and b"frame 4194304" in err()

    n = C.c_int32(7)
    M = (C.c_double * 16)(*np.eye(4).reshape(-1))
    assert lib.velo_build_matches(None, 1, 0, None, None, None, 0, C.byref(n)) == -1 and b"null ctx" in err()
    assert lib.velo_build_matches(fake, -1, 0, None, None, None, 0, C.byref(n)) == -1 and b"frame -1" in err()
    assert lib.velo_build_matches(fake, 1, 1 << 22, None, None, None, 0, C.byref(n)) == -1 and b"frame 4194304" in err()
    assert lib.velo_build_matches(fake, 1, 0, None, None, None, -1, C.byref(n)) == -1 and b"negative capacity" in err()
    assert lib.velo_build_matches(fake, 1, 0, None, None, None, 0, None) == -1 and b"null n_out" in err()
    M[7] = float("inf")
    assert lib.velo_build_matches(fake, 1, 0, M, None, None, 0, C.byref(n)) == -1 and b"pose2_inv[7] is not finite" in err()
    fr = np.zeros(2, dtype=np.int32)
    no = np.zeros(2, dtype=np.int32)
    vp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    arr = (C.c_void_p * 2)(fake, fake)
    assert lib.velo_build_matches_batch(C.cast(arr, C.c_void_p), 2, vp(fr), vp(fr), None, None, None, 0, vp(no)) == -1 and b"same context" in err()
    arr = (C.c_void_p * 2)(fake, None)
    assert lib.velo_build_matches_batch(C.cast(arr, C.c_void_p), 2, vp(fr), vp(fr), None, None, None, 0, vp(no)) == -1 and b"null" in err()
    assert lib.velo_build_matches_batch(C.cast(arr, C.c_void_p), 0, vp(fr), vp(fr), None, None, None, 0, vp(no)) == -1 and b"0 contexts" in err()
    arr = (C.c_void_p * 2)(fake, C.c_void_p(0x2000))
    assert lib.velo_build_matches_batch(C.cast(arr, C.c_void_p), 2, None, vp(fr), None, None, None, 0, vp(no)) == -1 and b"null frames" in err()
    assert lib.velo_build_matches_batch(None, 2, vp(fr), vp(fr), None, None, None, 0, vp(no)) == -1 and b"null context list" in err()

    assert lib.velo_get_visual(None, None, 0, C.byref(n)) == -1 and b"null ctx" in err()
    assert lib.velo_get_visual(fake, None, 0, None) == -1 and b"null n" in err()
    assert lib.velo_get_visual(fake, None, -1, C.byref(n)) == -1 and b"negative capacity" in err()
