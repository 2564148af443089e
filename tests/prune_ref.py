"""removeSlightlyLessTerribleFeatures (velo.h:272-327) for one camera of one frame, restated twice: prune_literal() is the reference's
loop with Python containers (the std::set, the walk over i with j and jd++, push_back on the new cloud), prune_vectorised() the
`a = a[indices]` form its comment wishes for.  A camera is the tuple (ids [n], keypoints [n, 2], has_depth [n], kp_with_depth [m, 3])
of visual_ref / landmarks_ref; rows is uint8 [n, 64] or None (an entry without descriptor rows).  Both return
(camera, rows, kept) with kept the old indices that stay, ascending -- what the caller applies to keypoints_p."""
import numpy as np


def prune_literal(cam, rows, good_first):
    """velo.h:287-325; good_first: gm.first of every good match of this camera, any order, duplicates as they come"""
    ids, kps, has, cloud = cam
    good_indices = set()
    for first in good_first:
        good_indices.add(int(first))
    m, n = len(good_indices), len(ids)
    tmp_keypoints = np.zeros((m, 2), dtype=np.float32)
    tmp_ids = np.zeros(m, dtype=np.int32)
    tmp_rows = None if rows is None else np.zeros((m, 64), dtype=np.uint8)
    tmp_has_depth = np.zeros(m, dtype=np.int32)
    tmp_cloud = []
    kept = []
    j = jd = 0
    for i in range(n):
        if i not in good_indices:
            continue
        tmp_keypoints[j] = kps[i]
        tmp_ids[j] = ids[i]
        if rows is not None:
            tmp_rows[j] = rows[i]
        d = int(has[i])
        if d != -1:
            tmp_cloud.append(np.asarray(cloud, dtype=np.float32).reshape(-1, 3)[d])
            tmp_has_depth[j] = jd
            jd += 1
        else:
            tmp_has_depth[j] = -1
        kept.append(i)
        j += 1
    assert j == m, "good_matches names a keypoint the frame does not hold"
    new_cloud = np.array(tmp_cloud, dtype=np.float32).reshape(-1, 3)
    return (tmp_ids, tmp_keypoints, tmp_has_depth, new_cloud), tmp_rows, np.asarray(kept, dtype=np.int32)


def prune_vectorised(cam, rows, good_first):
    """the same without a loop over keypoints"""
    ids, kps, has, cloud = [np.asarray(a) for a in cam]
    kept = np.unique(np.asarray(good_first, dtype=np.int64)).astype(np.int32)
    old = has[kept].astype(np.int64)
    with_depth = old != -1
    new_has = np.full(len(kept), -1, dtype=np.int32)
    new_has[with_depth] = np.arange(int(with_depth.sum()), dtype=np.int32)
    new_cloud = np.asarray(cloud, dtype=np.float32).reshape(-1, 3)[old[with_depth]]
    return ((ids[kept].astype(np.int32), kps[kept].astype(np.float32).reshape(-1, 2), new_has, new_cloud),
            None if rows is None else np.asarray(rows, dtype=np.uint8)[kept], kept)


def same(a, b):
    """two (camera, rows, kept) results are byte-equal"""
    (ca, ra, ka), (cb, rb, kb) = a, b
    if (ra is None) != (rb is None) or (ra is not None and ra.tobytes() != rb.tobytes()):
        return False
    return ka.tobytes() == kb.tobytes() and all(np.ascontiguousarray(x).tobytes() == np.ascontiguousarray(y).tobytes() and x.shape == y.shape
                                                for x, y in zip(ca, cb))


def make_camera(rng, n, mode="mixed", with_rows=True):
    """n keypoints with distinct ids; has_depth by mode: 'mixed' (about half, slots permuted), 'none' (all -1), 'all' (all set, slots
    permuted), 'shared' (one depth point that every keypoint names)"""
    ids = rng.permutation(4 * n + 8)[:n].astype(np.int32)
    kps = (rng.normal(size=(n, 2)) * 0.3).astype(np.float32)
    if mode == "shared":
        has = np.zeros(n, dtype=np.int32)
        cloud = (rng.normal(size=(1, 3)) * 5 + [0, 0, 20]).astype(np.float32)
    else:
        w = np.flatnonzero(rng.random(n) < {"mixed": 0.5, "none": -1.0, "all": 2.0}[mode])
        has = np.full(n, -1, dtype=np.int32)
        has[w] = rng.permutation(len(w)).astype(np.int32)
        cloud = (rng.normal(size=(len(w), 3)) * 5 + [0, 0, 20]).astype(np.float32)
    rows = rng.integers(0, 256, size=(n, 64), dtype=np.uint8) if with_rows else None
    return (ids, kps, has, cloud), rows


def keep_sets(rng, n):
    """{name: index list} of the keep sets the tests walk for an entry of n keypoints; 'half' is unsorted and holds duplicates"""
    half = rng.permutation(n)[:(n + 1) // 2]
    out = {"none": [], "all": list(range(n)), "every_second": list(range(0, n, 2)), "first": [0] if n else [], "last": [n - 1] if n else [],
           "half": rng.permutation(np.r_[half, half[:len(half) // 3]]).tolist()}
    return {k: np.asarray(v, dtype=np.int32) for k, v in out.items()}
