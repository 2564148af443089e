"""The visual set frameToFrame works on, restated from the reference with Python containers: matchUsingId (velo.h:562-590, a dict where
the reference has its std::map id2ind), the per-match gather of velo.h:627-654 and the landmark rule of velo.h:634-644 (a dict
id -> point where the reference has the std::map landmarks_at_frame; landmarks_dict() fills it from
LandmarkBook.landmarks_at_frame).  assemble() emits the records as an api.MATCH_DTYPE array in the order the adaptor's loop
pushes them: camera-major, matches in matchUsingId's order.  Also here: a second, vectorised numpy form of the same rules and
the seeded inputs the assembly tests share.  A frame's camera is the tuple (ids, keypoints [n, 2], has_depth [n],
kp_with_depth [m, 3]) that landmarks_ref.sequence produces."""
import numpy as np

import landmarks_ref as LR
from velo_amd import api

CHUNK = 256          # entries of frame2 per workgroup of the compaction (kFrChunk): the sizes around it are test cases


def match_using_id(ids1, ids2):
    """velo.h:570-579 for one camera"""
    id2ind = {}
    for ind in range(len(ids1)):
        id2ind[int(ids1[ind])] = ind
    matches = []
    for ind in range(len(ids2)):
        id = int(ids2[ind])
        if id in id2ind:
            matches.append((id2ind[id], ind))
    return matches


def landmarks_dict(book, pose_inv, frame2):
    """main.cpp:376-386: the std::map getLandmarksAtFrame returns for frame2"""
    ids, xyz = book.landmarks_at_frame(pose_inv, frame2)
    return {int(i): p for i, p in zip(ids, xyz)}


def assemble(frame1, frame2, cam_trans, landmarks_at_frame=None):
    """velo.h:622-654 with matches = matchUsingId(frame1, frame2): (records, matches per camera).  frame1 / frame2: per camera
    (ids, keypoints, has_depth, kp_with_depth); landmarks_at_frame: {id: float32[3]} or None (an empty map)."""
    lm = landmarks_at_frame or {}
    recs, per_cam = [], []
    for cam in range(len(frame1)):
        ids1, kp1, has1, cl1 = frame1[cam]
        ids2, kp2, has2, cl2 = frame2[cam]
        mc = match_using_id(ids1, ids2)
        per_cam.append(len(mc))
        for point1, point2 in mc:
            id = int(ids2[point2])
            d1, d2 = has1[point1] != -1, has2[point2] != -1
            m = np.zeros((), dtype=api.MATCH_DTYPE)
            if id in lm:
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
    return out, np.asarray(per_cam, dtype=np.int32)


def assemble_vectorised(frame1, frame2, cam_trans, landmarks_at_frame=None):
    """The same records without a loop over matches: sorting and searching where assemble() walks a dict."""
    lm = landmarks_at_frame or {}
    lm_ids = np.array(sorted(lm), dtype=np.int64)
    lm_xyz = np.array([lm[i] for i in sorted(lm)], dtype=np.float32).reshape(-1, 3)
    parts, per_cam = [], []
    for cam in range(len(frame1)):
        ids1, kp1, has1, cl1 = [np.asarray(a) for a in frame1[cam]]
        ids2, kp2, has2, cl2 = [np.asarray(a) for a in frame2[cam]]
        n1, n2 = len(ids1), len(ids2)
        out = np.zeros(0, dtype=api.MATCH_DTYPE)
        if n1 and n2:
            order = np.lexsort((np.arange(n1), ids1))                 # by id, then by index: the last of a run is the last index
            s = ids1[order]
            last = np.r_[s[1:] != s[:-1], True]
            uid, uind = s[last], order[last]
            pos = np.searchsorted(uid, ids2)
            hit = (pos < len(uid)) & (uid[np.minimum(pos, len(uid) - 1)] == ids2)
            p2 = np.flatnonzero(hit)
            p1 = uind[pos[p2]]
            out = np.zeros(len(p2), dtype=api.MATCH_DTYPE)
            h1, h2 = has1[p1], has2[p2]
            if len(lm_ids):
                lpos = np.searchsorted(lm_ids, ids2[p2])
                is_lm = (lpos < len(lm_ids)) & (lm_ids[np.minimum(lpos, len(lm_ids) - 1)] == ids2[p2])
            else:
                lpos, is_lm = np.zeros(len(p2), dtype=np.int64), np.zeros(len(p2), dtype=bool)
            dep2 = ~is_lm & (h2 != -1)
            out["p3_2"][is_lm] = lm_xyz[lpos[is_lm]]
            out["p3_2"][dep2] = np.asarray(cl2, dtype=np.float32).reshape(-1, 3)[h2[dep2]]
            out["p3_1"][h1 != -1] = np.asarray(cl1, dtype=np.float32).reshape(-1, 3)[h1[h1 != -1]]
            out["p2_1"], out["p2_2"] = kp1[p1], kp2[p2]
            out["t_cam"] = cam_trans[cam]
            out["cam"], out["point1"], out["point2"] = cam, p1, p2
            out["d1"], out["d2"] = h1 != -1, is_lm | (h2 != -1)
        parts.append(out)
        per_cam.append(len(out))
    return np.concatenate(parts) if parts else np.zeros(0, dtype=api.MATCH_DTYPE), np.asarray(per_cam, dtype=np.int32)


def random_camera(rng, n, id_pool, p_depth=0.5):
    """n keypoints with distinct ids drawn from id_pool, about p_depth of them with a depth point, the cloud in shuffled order"""
    ids = rng.choice(np.asarray(id_pool), size=n, replace=False).astype(np.int32) if n else np.zeros(0, np.int32)
    kps = rng.normal(size=(n, 2)).astype(np.float32) * np.float32(0.3)
    with_depth = np.flatnonzero(rng.random(n) < p_depth)
    has = np.full(n, -1, dtype=np.int32)
    has[with_depth] = rng.permutation(len(with_depth)).astype(np.int32)
    cloud = (rng.normal(size=(len(with_depth), 3)) * 5 + [0, 0, 20]).astype(np.float32)
    return ids, kps, has, cloud


def random_pair(seed, sizes1, sizes2, id_hi=None, p_depth=0.5):
    """(frame1, frame2, cam_trans) with sizes1[cam] / sizes2[cam] keypoints; about 80 % of the smaller side's ids are shared"""
    rng = np.random.default_rng(seed)
    f1, f2 = [], []
    for n1, n2 in zip(sizes1, sizes2):
        hi = id_hi or max(4 * max(n1, n2), 16)
        a = random_camera(rng, n1, np.arange(hi), p_depth)
        share = a[0][rng.random(n1) < 0.8][:n2]
        rest = np.setdiff1d(np.arange(hi, 2 * hi), share)
        b = list(random_camera(rng, n2, rest, p_depth))
        b[0][:len(share)] = share
        perm = rng.permutation(n2)
        b[0] = b[0][perm]
        f1.append(a)
        f2.append(tuple(b))
    ct = (rng.normal(size=(len(sizes1), 3)) * 0.3).astype(np.float32)
    return f1, f2, ct


def id_cases():
    """Hand-placed ids, one camera: frame1 holds id 7 twice and id 9 three times (the last index wins), frame2 holds id 11 twice
    (two matches) and id 9 twice; ids 1, 2 only in frame1, 3, 4 only in frame2; ids 5 and 70000 on both sides; ids 80000 and
    90000, beyond any landmark store the tests build, on both sides."""
    rng = np.random.default_rng(99)
    ids1 = np.array([7, 1, 9, 5, 7, 9, 11, 70000, 2, 9, 80000, 90000], dtype=np.int32)
    ids2 = np.array([11, 3, 9, 70000, 11, 4, 7, 5, 9, 90000, 80000], dtype=np.int32)

    def cam(ids):
        n = len(ids)
        has = np.array([k // 2 if k % 2 == 0 else -1 for k in range(n)], dtype=np.int32)
        return ids, rng.normal(size=(n, 2)).astype(np.float32), has, rng.normal(size=((n + 1) // 2, 3)).astype(np.float32)
    return [cam(ids1)], [cam(ids2)], np.array([[0.1, -0.2, 0.3]], dtype=np.float32)


def landmark_case():
    """A short landmarks_ref.sequence drive (2 cameras, 8 frames, 420 ids): frames 0..5 are observed and triangulated, then frame 6
    (frame1) is registered against frame 5 (frame2).  Returns the sequence and the pair."""
    ids = list(range(0, 420))
    seq = LR.sequence(31, 8, 2, ids, first_frame={i: ((i * 5 + 3) % 7, 2 + (i * 3) % 6) for i in ids})
    return seq, 6, 5


def walk_book(seq, upto, solve=None):
    """main.cpp:614-679 for frames 0..upto on a LandmarkBook.  solve(frame, ids) -> points gives the triangulated points (the GPU test
    hands the device's); without it every landmark gets a made-up point, which is all the CPU occurrence counts need."""
    book = LR.LandmarkBook(seq["n_cams"])
    for f in range(upto + 1):
        pc = seq["frames"][f]
        book.observe_frame(f, [c[1] for c in pc], [c[0] for c in pc], [c[2] for c in pc], [c[3] for c in pc])
        ids = book.ids_to_triangulate(f)
        pts = solve(f, ids) if solve else np.array([[0.01 * i, -0.02 * i, 10.0 + (i % 13)] for i in ids], dtype=np.float32)
        if ids:
            book.store(ids, pts)
    return book


def occurrence_counts(frame1, frame2, landmarks_at_frame):
    """per camera: {(d1, d2): count}, landmark-replaces-depth count, landmark-where-no-depth count"""
    out = []
    for cam in range(len(frame1)):
        ids2, has1, has2 = frame2[cam][0], frame1[cam][2], frame2[cam][2]
        combos = {(a, b): 0 for a in (0, 1) for b in (0, 1)}
        replaced = fresh = 0
        for p1, p2 in match_using_id(frame1[cam][0], ids2):
            is_lm = int(ids2[p2]) in landmarks_at_frame
            d1, d2 = int(has1[p1] != -1), int(has2[p2] != -1 or is_lm)
            combos[(d1, d2)] += 1
            replaced += int(is_lm and has2[p2] != -1)
            fresh += int(is_lm and has2[p2] == -1)
        out.append((combos, replaced, fresh))
    return out
