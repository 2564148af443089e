"""The CHECKER of the descriptor matcher (velo_match_descriptors): restatements of the reference's matchFeatures (velo.h:499-560) for
64-byte (FREAK, 512-bit) descriptors.  Two forms:

  match_scalar   a literal, row-by-row transcription of the non-CUDA branch (cv::BFMatcher(NORM_HAMMING).match, velo.h:527-531) and the
                 filter after it (velo.h:536-549), plain Python loops -- the pin;
  match          the same in vectorised numpy (np.bitwise_count on u64 views, chunked), fast enough for 20,000 x 3,000;
                 tests/test_descriptor_ref.py holds it to the scalar form.

Distances are integers, so both are exact.  Ties: the LOWEST train index, as the strict `<` scan of cv::BFMatcher; the CUDA branch
(velo.h:517-525) does not pin its order on ties.  min_dist is reported as -1 where the reference's stays at 1e9
(no match at all: an empty query or train set), in which case nothing is kept either way."""
import numpy as np

MATCH_THRESH = 29.0          # kitti.h:27


def _rows(a):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.uint8))
    return a.reshape(0, 64) if a.size == 0 else a


def match_scalar(query, train, match_thresh=MATCH_THRESH):
    """(train_idx [nq], distance [nq], min_dist, pairs [k, 2]) by plain loops."""
    q, t = _rows(query), _rows(train)
    mc = []                                                    # velo.h:516  std::vector<cv::DMatch> mc
    if len(t) > 0:                                             # cv::BFMatcher::match: no train rows, no matches
        for qi in range(len(q)):
            best_d, best_t = None, -1
            for ti in range(len(t)):
                d = sum(bin(int(a) ^ int(b)).count("1") for a, b in zip(q[qi], t[ti]))   # NORM_HAMMING
                if best_d is None or d < best_d:               # strict `<`: the first (lowest) index of equal distances stays
                    best_d, best_t = d, ti
            mc.append((qi, best_t, best_d))                    # DMatch(queryIdx, trainIdx, distance), query order
    min_dist = 1e9                                             # velo.h:536
    for _, _, d in mc:                                         # velo.h:537-540
        if d < min_dist:
            min_dist = d
    pairs = []
    for qi, ti, d in mc:                                       # velo.h:545-548
        if d > max(1.5 * min_dist, match_thresh):
            continue
        pairs.append((qi, ti))
    idx = np.full(len(q), -1, np.int32)
    dist = np.full(len(q), -1, np.int32)
    for qi, ti, d in mc:
        idx[qi], dist[qi] = ti, d
    md = int(min_dist) if mc else -1
    return idx, dist, md, np.asarray(pairs, np.int32).reshape(-1, 2)


def distances(query, train, chunk=512):
    """[nq, nt] int32 Hamming distances, chunked over the queries (np.bitwise_count on u64 views)."""
    q, t = _rows(query).view(np.uint64), _rows(train).view(np.uint64)    # [n, 8]
    out = np.empty((len(q), len(t)), np.int32)
    for a in range(0, len(q), chunk):
        x = q[a:a + chunk, None, :] ^ t[None, :, :]
        out[a:a + chunk] = np.bitwise_count(x).sum(axis=2, dtype=np.int32)
    return out


def match(query, train, match_thresh=MATCH_THRESH, chunk=512):
    """The same result as match_scalar, vectorised; the distance matrix is never held whole."""
    q, t = _rows(query), _rows(train)
    nq, nt = len(q), len(t)
    idx = np.full(nq, -1, np.int32)
    dist = np.full(nq, -1, np.int32)
    if nq == 0 or nt == 0:
        return idx, dist, -1, np.zeros((0, 2), np.int32)
    for a in range(0, nq, chunk):
        D = distances(q[a:a + chunk], t, chunk)
        idx[a:a + chunk] = np.argmin(D, axis=1)                 # argmin returns the first of equal minima: the lowest index
        dist[a:a + chunk] = D[np.arange(len(D)), idx[a:a + chunk]]
    md = int(dist.min())
    keep = ~(dist.astype(np.float64) > max(1.5 * md, float(match_thresh)))
    qi = np.nonzero(keep)[0].astype(np.int32)
    return idx, dist, md, np.stack([qi, idx[qi]], axis=1).astype(np.int32).reshape(-1, 2)


def match_jobs(jobs, match_thresh=MATCH_THRESH):
    """match() for every (query, train) pair: lists of train_idx, distance, pairs and the min_dist array"""
    res = [match(q, t, match_thresh) for q, t in jobs]
    return [r[0] for r in res], [r[1] for r in res], np.asarray([r[2] for r in res], np.int32), [r[3] for r in res]
