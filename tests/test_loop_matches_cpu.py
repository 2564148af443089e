"""CPU checks of the loop-closure match assembly's boundary: tests/loop_ref.py (descriptor_ref.match per camera + the gather of
velo.h:627-654) against an independent form (on frames whose descriptors are one distinct row per id, descriptor matching IS
matchUsingId, so visual_ref gives the same records) and against hand-built cases; the occurrence conditions that keep the GPU
tests on the shared seeded input from passing vacuously; and the argument validation of velo_frames_put_descriptors,
velo_frames_desc_info, velo_build_matches_desc[_batch] and velo_match_frames, which refuse bad arguments with the library's usual
argument error before any context is touched (no GPU needed; "n differs from the entry's keypoint count" needs a live context and
is checked in tests/test_gpu_loop_matches.py)."""
import ctypes as C

import numpy as np
import pytest

import descriptor_ref as DR
import loop_ref as LP
import visual_ref as VR
import velo_amd  # noqa: F401
from velo_amd import api, build


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return api.load_library()


def by_cam_point1(recs):
    return recs[np.lexsort((recs["point1"], recs["cam"]))]


def test_restatement_equals_match_using_id_on_one_distinct_row_per_id():
    seq, fr1, fr2 = VR.landmark_case()
    book = VR.walk_book(seq, fr2)
    lm = VR.landmarks_dict(book, np.linalg.inv(api.pose_vec_to_mat(seq["poses"][fr2])), fr2)
    cases = [(seq["frames"][fr1], seq["frames"][fr2], seq["cam_trans"], lm)]
    for sizes in (((300, 500), (0, 512)), ((700,), (769,)), ((1,), (1,))):
        cases.append(VR.random_pair(11 + sum(sizes[0]), sizes[0], sizes[1]) + (None,))
    n_records = 0
    for f1, f2, ct, lm in cases:
        rows = LP.rows_by_id(3, [c[0] for c in f1] + [c[0] for c in f2])
        d1, d2 = rows[:len(f1)], rows[len(f1):]
        pairs, md = LP.match_cameras(d1, d2)
        for cam in range(len(f1)):
            assert len(set(f1[cam][0].tolist())) == len(f1[cam][0]) and len(set(f2[cam][0].tolist())) == len(f2[cam][0])   # duplicate-free ids
            want = set(VR.match_using_id(f1[cam][0], f2[cam][0]))
            assert set(map(tuple, pairs[cam].tolist())) == want
            assert md[cam] == (0 if want else md[cam])
        got, n, _ = LP.assemble(f1, f2, d1, d2, ct, lm)
        ref, n_ref = VR.assemble(f1, f2, ct, lm)
        assert n.tolist() == n_ref.tolist()
        assert by_cam_point1(got).tobytes() == by_cam_point1(ref).tobytes()
        n_records += len(got)
    assert n_records > 1000


def test_hand_built_cases():
    rng = np.random.default_rng(7)
    base = LP.rand_rows(rng, 6)
    cam = lambda n: VR.random_camera(rng, n, np.arange(100))   # noqa: E731
    ct = np.float32([[.1, .2, .3]])
    # a tie: train rows 1 and 4 are identical, the lowest index wins; queries 0 and 2 keep the same train row: two records
    t = base[[0, 1, 2, 3, 1]]
    q = np.stack([base[1], base[3], LP.flip_bits(rng, base[1:2], [3])[0]])
    f1, f2 = [cam(3)], [cam(5)]
    recs, n, md = LP.assemble(f1, f2, [q], [t], ct)
    assert LP.pairs_of(recs).tolist() == [[0, 1], [1, 3], [2, 1]] and n.tolist() == [3] and md.tolist() == [0]
    assert recs["p2_2"][0].tolist() == recs["p2_2"][2].tolist() == f2[0][1][1].tolist() and recs["p2_1"][2].tolist() == f1[0][1][2].tolist()
    assert recs["t_cam"][1].tolist() == ct[0].tolist() and not recs["pad"].any()
    # the filter drops everything but the minimum: min_dist 40 gives the bound max(60, 29) and every other query is ~200 bits away
    q = np.concatenate([LP.flip_bits(rng, base[2:3], [40]), LP.rand_rows(rng, 4)])
    recs, n, md = LP.assemble([cam(5)], f2, [q], [t], ct)
    assert LP.pairs_of(recs).tolist() == [[0, 2]] and md.tolist() == [40]
    # an empty query set and an empty train set, next to a camera that matches
    f1, f2 = [cam(0), cam(4), cam(2)], [cam(3), cam(0), cam(2)]
    d1 = [np.zeros((0, 64), np.uint8), base[:4], base[:2]]
    d2 = [base[:3], np.zeros((0, 64), np.uint8), base[[1, 0]]]
    recs, n, md = LP.assemble(f1, f2, d1, d2, np.float32(np.arange(9).reshape(3, 3)))
    assert n.tolist() == [0, 0, 2] and md.tolist() == [-1, -1, 0] and recs["cam"].tolist() == [2, 2] and LP.pairs_of(recs).tolist() == [[0, 1], [1, 0]]
    # the landmark rule on a descriptor match: id = frame2's id at point2
    f1, f2 = [cam(2)], [cam(2)]
    lm = {int(f2[0][0][1]): np.float32([1, 2, 3])}
    recs, _, _ = LP.assemble(f1, f2, [base[:2]], [base[[1, 0]]], ct, lm)
    assert LP.pairs_of(recs).tolist() == [[0, 1], [1, 0]] and recs["p3_2"][0].tolist() == [1, 2, 3] and recs["d2"][0] == 1


def test_inputs_hold_the_cases_the_gpu_test_relies_on():
    seq, fr1, fr2, desc = LP.landmark_case()
    f1, f2 = seq["frames"][fr1], seq["frames"][fr2]
    book = VR.walk_book(seq, fr2)
    lm = VR.landmarks_dict(book, np.eye(4), fr2)
    pairs, md = LP.match_cameras(desc[fr1], desc[fr2])
    assert len(f1) == 2
    for cam, (combos, replaced, fresh) in enumerate(LP.occurrence_counts(f1, f2, pairs, lm)):
        kept = len(pairs[cam])
        assert kept >= 20 and len(desc[fr1][cam]) - kept >= 20, (kept, len(desc[fr1][cam]))
        assert all(v >= 5 for v in combos.values()), combos
        assert replaced >= 5 and fresh >= 5, (replaced, fresh)
        trains, counts = np.unique(pairs[cam][:, 1], return_counts=True)
        assert (counts >= 2).any()                                       # a train row kept by two queries
        assert len(desc[fr1][cam]) == len(f1[cam][0]) and len(desc[fr2][cam]) == len(f2[cam][0])
    # the sized pairs keep and drop as well
    f1, f2, d1, d2, ct = LP.random_pair(5, (300, 65), (257, 300))
    pairs, md = LP.match_cameras(d1, d2)
    assert all(20 <= len(p) <= len(q) - 20 for p, q in zip(pairs, d1)) and (md >= 0).all()


def test_exports(lib):
    for name in ("velo_frames_put_descriptors", "velo_frames_desc_info", "velo_build_matches_desc", "velo_build_matches_desc_batch",
                 "velo_match_frames"):
        assert hasattr(lib, name) and name in api.SIGNATURES
    for name in ("frames_put_descriptors", "frames_desc_info", "build_matches_desc", "match_frames"):
        assert hasattr(api.Context, name)
    assert callable(api.build_matches_desc_batch)


def test_argument_validation_without_gpu(lib):
    fake = C.c_void_p(0x1000)                       # never dereferenced: every argument is checked before the context is touched
    err = lib.velo_last_error
    rows = (C.c_uint8 * 128)()
    assert lib.velo_frames_put_descriptors(None, 0, 0, rows, 2) == -1 and b"null ctx" in err()
    assert lib.velo_frames_put_descriptors(fake, -1, 0, rows, 2) == -1 and b"frame -1" in err()
    assert lib.velo_frames_put_descriptors(fake, 1 << 22, 0, rows, 2) == -1 and b"frame 4194304" in err()
    assert lib.velo_frames_put_descriptors(fake, 0, 8, rows, 2) == -1 and b"camera 8" in err()
    assert lib.velo_frames_put_descriptors(fake, 0, -1, rows, 2) == -1 and b"camera -1" in err()
    assert lib.velo_frames_put_descriptors(fake, 0, 0, rows, -2) == -1 and b"negative count" in err()
    assert lib.velo_frames_put_descriptors(fake, 0, 0, None, 2) == -1 and b"null descriptor rows" in err()
    assert lib.velo_frames_put_descriptors(fake, 0, 0, rows, (1 << 22) + 1) == -1 and b"indexes at most" in err()
    assert lib.velo_frames_desc_info(None, None) == -1 and lib.velo_frames_desc_info(fake, None) == -1 and b"null argument" in err()

    n = C.c_int32(7)
    nan, inf = float("nan"), float("inf")
    M = (C.c_double * 16)(*np.eye(4).reshape(-1))
    bm = lib.velo_build_matches_desc
    assert bm(None, 1, 0, None, 29.0, None, None, 0, C.byref(n)) == -1 and b"null ctx" in err()
    assert bm(fake, -1, 0, None, 29.0, None, None, 0, C.byref(n)) == -1 and b"frame -1" in err()
    assert bm(fake, 1, 1 << 22, None, 29.0, None, None, 0, C.byref(n)) == -1 and b"frame 4194304" in err()
    assert bm(fake, 1, 0, None, 29.0, None, None, -1, C.byref(n)) == -1 and b"negative capacity" in err()
    assert bm(fake, 1, 0, None, 29.0, None, None, 0, None) == -1 and b"null n_out" in err()
    assert bm(fake, 1, 0, None, nan, None, None, 0, C.byref(n)) == -1 and b"match_thresh is NaN" in err()
    M[7] = inf
    assert bm(fake, 1, 0, M, 29.0, None, None, 0, C.byref(n)) == -1 and b"pose2_inv[7] is not finite" in err()
    fr = np.zeros(2, dtype=np.int32)
    no = np.zeros(2, dtype=np.int32)
    vp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    bb = lib.velo_build_matches_desc_batch
    arr = (C.c_void_p * 2)(fake, fake)
    assert bb(C.cast(arr, C.c_void_p), 2, vp(fr), vp(fr), None, 29.0, None, None, 0, vp(no)) == -1 and b"same context" in err()
    arr = (C.c_void_p * 2)(fake, None)
    assert bb(C.cast(arr, C.c_void_p), 2, vp(fr), vp(fr), None, 29.0, None, None, 0, vp(no)) == -1 and b"null" in err()
    assert bb(C.cast(arr, C.c_void_p), 0, vp(fr), vp(fr), None, 29.0, None, None, 0, vp(no)) == -1 and b"0 contexts" in err()
    assert bb(C.cast(arr, C.c_void_p), -3, vp(fr), vp(fr), None, 29.0, None, None, 0, vp(no)) == -1 and b"-3 contexts" in err()
    arr = (C.c_void_p * 2)(fake, C.c_void_p(0x2000))
    assert bb(C.cast(arr, C.c_void_p), 2, None, vp(fr), None, 29.0, None, None, 0, vp(no)) == -1 and b"null frames" in err()
    assert bb(C.cast(arr, C.c_void_p), 2, vp(fr), vp(fr), None, nan, None, None, 0, vp(no)) == -1 and b"match_thresh is NaN" in err()
    assert bb(None, 2, vp(fr), vp(fr), None, 29.0, None, None, 0, vp(no)) == -1 and b"null context list" in err()

    out = np.zeros(8, dtype=np.int32)
    mf = lib.velo_match_frames
    assert mf(None, 0, vp(fr), 2, 29.0, vp(out), vp(out)) == -1 and b"null ctx" in err()
    assert mf(fake, 0, vp(fr), -1, 29.0, vp(out), vp(out)) == -1 and b"negative candidate count" in err()
    assert mf(fake, 0, vp(fr), 2, nan, vp(out), vp(out)) == -1 and b"match_thresh is NaN" in err()
    assert mf(fake, -4, vp(fr), 2, 29.0, vp(out), vp(out)) == -1 and b"frame -4" in err()
    assert mf(fake, 0, None, 0, 29.0, None, None) == 0                                  # no candidates: nothing to do
    assert mf(fake, 0, None, 2, 29.0, vp(out), vp(out)) == -1 and b"null frames2" in err()
    assert mf(fake, 0, vp(fr), 2, 29.0, None, vp(out)) == -1 and mf(fake, 0, vp(fr), 2, 29.0, vp(out), None) == -1
    fr[1] = -9
    assert mf(fake, 0, vp(fr), 2, 29.0, vp(out), vp(out)) == -1 and b"candidate 1: frame -9" in err()
