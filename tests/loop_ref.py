"""The visual set of a loop-closure edge (main.cpp:359: matchFeatures in place of matchUsingId), restated from the reference:
descriptor_ref.match per camera (cv::BFMatcher(NORM_HAMMING).match with query = frame1's rows and train = frame2's, the lowest
train index on ties, and the filter of velo.h:536-549), then the per-match gather of velo.h:627-654 for an arbitrary match list with
the dict-based landmark rule of visual_ref.assemble (which fixes matchUsingId as its match list and is therefore restated here).
Records are api.MATCH_DTYPE, camera-major, in query order.  Also here: the seeded inputs the loop-closure tests share.  A frame's
camera is visual_ref's tuple (ids, keypoints [n, 2], has_depth [n], kp_with_depth [m, 3]); its descriptors are a uint8 (n, 64)
array per camera."""
import numpy as np

import descriptor_ref as DR
import visual_ref as VR
from velo_amd import api


def gather(frame1, frame2, matches, cam_trans, landmarks_at_frame=None):
    """velo.h:622-654 for matches[cam] = [(point1, point2), ...]: the records, camera-major in list order"""
    lm = landmarks_at_frame or {}
    recs = []
    for cam in range(len(frame1)):
        ids1, kp1, has1, cl1 = frame1[cam]
        ids2, kp2, has2, cl2 = frame2[cam]
        for point1, point2 in matches[cam]:
            point1, point2 = int(point1), int(point2)
            id = int(ids2[point2])                                      # velo.h:630
            d1, d2 = has1[point1] != -1, has2[point2] != -1
            m = np.zeros((), dtype=api.MATCH_DTYPE)
            if id in lm:                                                # velo.h:634-644
                m["p3_2"] = lm[id]
                d2 = True
            elif d2:
                m["p3_2"] = cl2[has2[point2]]
            if d1:
                m["p3_1"] = cl1[has1[point1]]
            m["p2_1"], m["p2_2"] = kp1[point1], kp2[point2]
            m["t_cam"] = cam_trans[cam]
            m["cam"], m["point1"], m["point2"] = cam, point1, point2
            m["d1"], m["d2"] = int(d1), int(d2)
            recs.append(m)
    out = np.zeros(len(recs), dtype=api.MATCH_DTYPE)
    for k, m in enumerate(recs):
        out[k] = m
    return out


def match_cameras(desc1, desc2, match_thresh=DR.MATCH_THRESH):
    """matchFeatures(descriptors, frame1, frame2, matches) (velo.h:551-560): per camera the kept pairs [k, 2] and min_dist (-1: none)"""
    res = [DR.match(q, t, match_thresh) for q, t in zip(desc1, desc2)]
    return [r[3] for r in res], np.asarray([r[2] for r in res], np.int32)


def assemble(frame1, frame2, desc1, desc2, cam_trans, landmarks_at_frame=None, match_thresh=DR.MATCH_THRESH):
    """(records, matches per camera, min_dist per camera) of frameToFrame(frame1, frame2) on the loop-closure branch"""
    pairs, md = match_cameras(desc1, desc2, match_thresh)
    return gather(frame1, frame2, pairs, cam_trans, landmarks_at_frame), np.asarray([len(p) for p in pairs], np.int32), md


def pairs_of(recs):
    return np.stack([recs["point1"], recs["point2"]], axis=1).astype(np.int32).reshape(-1, 2)


# ---- seeded inputs ---------------------------------------------------------------------------------------------------------------
def rand_rows(rng, n):
    return rng.integers(0, 256, (n, 64), dtype=np.uint8)


def flip_bits(rng, rows, flips):
    """rows with flips[i] distinct random bits of row i flipped"""
    bits = np.unpackbits(np.asarray(rows, np.uint8).reshape(-1, 64), axis=1, bitorder="little")
    for i, f in enumerate(flips):
        bits[i, rng.choice(512, size=int(f), replace=False)] ^= 1
    return np.packbits(bits, axis=1, bitorder="little")


def rows_by_id(seed, ids_per_cam):
    """a distinct random row per id: the descriptors of a frame whose keypoints are recognised exactly"""
    hi = max([int(np.max(i)) for i in ids_per_cam if len(i)] + [0]) + 1
    table = rand_rows(np.random.default_rng(seed), hi)
    assert len(np.unique(table, axis=0)) == hi
    return [table[np.asarray(i, np.int64)] if len(i) else np.zeros((0, 64), np.uint8) for i in ids_per_cam]


def random_pair(seed, sizes1, sizes2, p_depth=0.5):
    """visual_ref.random_pair with descriptors: frame2's rows are random, a row of frame1 is the row of frame2 that holds the same id with
    0-40 bits flipped (an id frame2 does not hold: a random row): (frame1, frame2, desc1, desc2, cam_trans)"""
    f1, f2, ct = VR.random_pair(seed, sizes1, sizes2, p_depth=p_depth)
    d1, d2 = near_rows(np.random.default_rng(seed + 1000), f1, f2)
    return f1, f2, d1, d2, ct


def near_rows(rng, frame1, frame2):
    """descriptors of two frames: frame2's rows are random, a row of frame1 is the row of frame2 that holds the same id (the last such
    row) with 0-40 bits flipped, or random when frame2 does not hold the id: (desc1, desc2)"""
    d1, d2 = [], []
    for a, b in zip(frame1, frame2):
        t = rand_rows(rng, len(b[0]))
        q = rand_rows(rng, len(a[0]))
        where = {int(i): k for k, i in enumerate(b[0])}
        hit = [k for k, i in enumerate(a[0]) if int(i) in where]
        if hit:
            q[hit] = flip_bits(rng, t[[where[int(a[0][k])] for k in hit]], rng.integers(0, 41, len(hit)))
        d1.append(q)
        d2.append(t)
    return d1, d2


def landmark_case():
    """visual_ref.landmark_case() with descriptors: (seq, frame1, frame2, desc) with desc[frame][cam] for the two frames.  A row of
    frame2 is its id's row; a row of frame1 is its id's row with 0-40 bits flipped; and in every camera the first three keypoints of
    frame1 whose id frame2 does not hold take the row (two bits flipped) of a train row that another query keeps."""
    seq, fr1, fr2 = VR.landmark_case()
    ids1 = [c[0] for c in seq["frames"][fr1]]
    ids2 = [c[0] for c in seq["frames"][fr2]]
    base = rows_by_id(41, ids1 + ids2)
    rng = np.random.default_rng(42)
    d1, d2 = [], base[len(ids1):]
    for cam, rows in enumerate(base[:len(ids1)]):
        flips = rng.integers(0, 41, len(rows))
        q = flip_bits(rng, rows, flips)
        where = {int(i): k for k, i in enumerate(ids2[cam])}
        lone = [k for k, i in enumerate(ids1[cam]) if int(i) not in where][:3]
        near = [where[int(i)] for k, i in enumerate(ids1[cam]) if int(i) in where and flips[k] <= 20][:3]    # train rows their own query keeps
        for k, t in zip(lone, near):
            q[k] = flip_bits(rng, d2[cam][t:t + 1], [2])[0]
        d1.append(q)
    return seq, fr1, fr2, {fr1: d1, fr2: d2}


def occurrence_counts(frame1, frame2, pairs, landmarks_at_frame):
    """visual_ref.occurrence_counts for a given match list: per camera {(d1, d2): count}, landmark-replaces-depth, landmark-where-no-depth"""
    out = []
    for cam in range(len(frame1)):
        ids2, has1, has2 = frame2[cam][0], frame1[cam][2], frame2[cam][2]
        combos = {(a, b): 0 for a in (0, 1) for b in (0, 1)}
        replaced = fresh = 0
        for p1, p2 in pairs[cam]:
            is_lm = int(ids2[p2]) in landmarks_at_frame
            combos[(int(has1[p1] != -1), int(has2[p2] != -1 or is_lm))] += 1
            replaced += int(is_lm and has2[p2] != -1)
            fresh += int(is_lm and has2[p2] == -1)
        out.append((combos, replaced, fresh))
    return out
