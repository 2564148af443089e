"""Numpy restatement of corner detection as the reference runs it (detectFeatures, velo.h:118-177): cv::GFTTDetector(3000, 0.001, 12),
i.e. cv::goodFeaturesToTrack(img, maxCorners, qualityLevel, minDistance, noArray(), blockSize = 3, useHarris = false), followed by
the reference's occupancy filter against the frame's existing points.  The GPU (velo_detect_features / velo_get_corner_response) is
held to this file bit for bit; tests/test_gftt_ref.py holds this file to independent sources.

The arithmetic is OpenCV 3.x (corner.cpp cornerMinEigenVal, featureselect.cpp) AS RECALLED -- no OpenCV here, DESIGN.md 2 -- with
one deliberate departure: OpenCV scales the Sobel derivatives to float before squaring and box-sums the products in float; this
restatement (order="exact") box-sums the integer products exactly (|dx| <= 1020, a 3 x 3 sum is <= 9 * 1020^2 < 2^24: exact in
int32 AND in float32) and applies the scale once, so the map does not depend on a summation order.  response(order="opencv_float")
keeps OpenCV's order for the parity budget.  Every float step below is a single IEEE f32 operation (no fusion).

Rules fixed here (unpinned): the map's maximum is clamped at 0 (a map without a positive value has no candidates);
equal values are ordered by the HIGHER row-major index first (OpenCV >= 3.4 sorts by address); existing points outside
[0, width) x [0, height) or non-finite take no part in the fresh test (the reference would index outside its grid).
"""
from __future__ import annotations

import numpy as np

f32 = np.float32
KSIZE = 3
BLOCK_SIZE = 3
SCALE = f32(1.0 / (255.0 * (1 << (KSIZE - 1)) * BLOCK_SIZE))     # cornerMinEigenVal's derivative scale for 8-bit input
SCALE2 = f32(SCALE * SCALE)                                       # one f32 product
MIN_DISTANCE_MAX = 64


def _pad101(a: np.ndarray, p: int = 1) -> np.ndarray:
    return np.pad(a, p, mode="reflect")                           # numpy "reflect" = OpenCV BORDER_REFLECT_101


def sobel(img: np.ndarray):
    """3 x 3 Sobel dx, dy of an 8-bit image in int64, reflect-101"""
    p = _pad101(np.asarray(img).astype(np.int64))
    h, w = img.shape
    sm_y = p[0:h, :] + 2 * p[1:h + 1, :] + p[2:h + 2, :]          # [1 2 1] down the rows
    sm_x = p[:, 0:w] + 2 * p[:, 1:w + 1] + p[:, 2:w + 2]          # [1 2 1] along the row
    dx = sm_y[:, 2:w + 2] - sm_y[:, 0:w]
    dy = sm_x[2:h + 2, :] - sm_x[0:h, :]
    return dx, dy


def box3(a: np.ndarray) -> np.ndarray:
    """un-normalised 3 x 3 box sum; the summed map itself is reflected (101) at the border"""
    p = _pad101(a)
    h, w = a.shape
    r = p[:, 0:w] + p[:, 1:w + 1] + p[:, 2:w + 2]
    return r[0:h] + r[1:h + 1] + r[2:h + 2]


def box_sums(img: np.ndarray):
    """(Sxx, Sxy, Syy) in int64, exact"""
    dx, dy = sobel(img)
    return box3(dx * dx), box3(dx * dy), box3(dy * dy)


def _tail(xx, xy, yy):
    """cornerMinEigenVal's calcMinEigenVal on float32 maps: a = xx/2, b = xy, c = yy/2; (a + c) - sqrt((a - c)^2 + b^2)"""
    a = xx * f32(0.5)
    b = xy
    c = yy * f32(0.5)
    d = a - c
    return ((a + c) - np.sqrt(d * d + b * b)).astype(np.float32)


def response(img: np.ndarray, order: str = "exact") -> np.ndarray:
    """the float32 map of cornerMinEigenVal(img, blockSize = 3, ksize = 3)"""
    if order == "exact":
        sxx, sxy, syy = box_sums(img)
        assert max(sxx.max(), syy.max(), np.abs(sxy).max()) < (1 << 24)
        return _tail(sxx.astype(np.float32) * SCALE2, sxy.astype(np.float32) * SCALE2, syy.astype(np.float32) * SCALE2)
    if order == "opencv_float":
        dx, dy = sobel(img)
        fx, fy = dx.astype(np.float32) * SCALE, dy.astype(np.float32) * SCALE

        def fbox(a):                                              # boxFilter: row sums, then column sums, f32, left to right
            p = _pad101(a)
            h, w = a.shape
            r = (p[:, 0:w] + p[:, 1:w + 1]) + p[:, 2:w + 2]
            return ((r[0:h] + r[1:h + 1]) + r[2:h + 2]).astype(np.float32)
        return _tail(fbox(fx * fx), fbox(fx * fy), fbox(fy * fy))
    raise ValueError(order)


def max_value(eig: np.ndarray) -> np.float32:
    return f32(max(float(eig.max()), 0.0)) if eig.size else f32(0)


def threshold(eig: np.ndarray, quality_level: float) -> np.float32:
    """maxVal * qualityLevel in double, handed to cv::threshold on a float image: rounded to f32"""
    return f32(np.float64(max_value(eig)) * np.float64(quality_level))


def candidate_mask(eig: np.ndarray, quality_level: float) -> np.ndarray:
    """THRESH_TOZERO (strict >), 3 x 3 dilation, value non-zero and equal to the dilated value, 1 <= x <= w - 2, 1 <= y <= h - 2"""
    h, w = eig.shape
    e = np.where(eig > threshold(eig, quality_level), eig, f32(0)).astype(np.float32)
    p = np.pad(e, 1, mode="constant", constant_values=-np.inf)
    dil = e.copy()
    for dy in range(3):
        for dx in range(3):
            dil = np.maximum(dil, p[dy:dy + h, dx:dx + w])
    m = (e != 0) & (e == dil)
    m[0, :] = m[-1, :] = False
    m[:, 0] = m[:, -1] = False
    return m


def candidates(eig: np.ndarray, quality_level: float, tie: str = "higher"):
    """(xs, ys, values) in the order of the sort: value descending, equal values by the higher (tie="higher") row-major index first"""
    h, w = eig.shape
    ys, xs = np.nonzero(candidate_mask(eig, quality_level))
    v = eig[ys, xs]
    idx = ys.astype(np.int64) * w + xs
    key2 = -idx if tie == "higher" else idx
    o = np.lexsort((key2, -v.astype(np.float64)))
    return xs[o].astype(np.int64), ys[o].astype(np.int64), v[o]


def select_scalar(xs, ys, w: int, h: int, min_distance: float, max_corners: int):
    """featureselect.cpp's loop, literally: a grid of cvRound(minDistance) cells, the 3 x 3 cells around a candidate searched for an
    accepted corner at dx^2 + dy^2 < minDistance^2; indices of the accepted candidates"""
    out = []
    if min_distance >= 1:
        cell = int(np.rint(min_distance))                          # cvRound
        gw, gh = (w + cell - 1) // cell, (h + cell - 1) // cell
        grid = [[] for _ in range(gw * gh)]
        md2 = float(min_distance) * float(min_distance)
        for i in range(len(xs)):
            x, y = int(xs[i]), int(ys[i])
            xc, yc = x // cell, y // cell
            x1, y1, x2, y2 = max(0, xc - 1), max(0, yc - 1), min(gw - 1, xc + 1), min(gh - 1, yc + 1)
            good = True
            for yy in range(y1, y2 + 1):
                for xx in range(x1, x2 + 1):
                    for (px, py) in grid[yy * gw + xx]:
                        ddx, ddy = float(x - px), float(y - py)
                        if ddx * ddx + ddy * ddy < md2:
                            good = False
                            break
                    if not good:
                        break
                if not good:
                    break
            if good:
                grid[yc * gw + xc].append((x, y))
                out.append(i)
                if max_corners > 0 and len(out) == max_corners:
                    break
    else:
        out = list(range(len(xs) if max_corners <= 0 else min(len(xs), max_corners)))
    return np.asarray(out, dtype=np.int64)


def _conflict_pairs(xs, ys, w: int, h: int, min_distance: float):
    """(lo, hi): every pair of candidates at squared distance < min_distance^2, lo = the one earlier in the order (larger key)"""
    n = len(xs)
    if n <= 4000:                                                  # few candidates: all pairs at once
        i, j = np.nonzero(np.triu((xs[:, None] - xs[None, :]) ** 2 + (ys[:, None] - ys[None, :]) ** 2 < float(min_distance) ** 2, 1))
        return i.astype(np.int64), j.astype(np.int64)
    idmap = np.full((h, w), -1, dtype=np.int64)
    idmap[ys, xs] = np.arange(n)
    md2 = float(min_distance) * float(min_distance)
    r = int(np.ceil(min_distance)) - 1
    lo, hi = [], []
    for dy in range(0, r + 1):
        for dx in range(-r, r + 1):
            if (dy == 0 and dx <= 0) or not (dx * dx + dy * dy < md2):
                continue
            a = idmap[0:h - dy, max(0, -dx):w - max(0, dx)]
            b = idmap[dy:h, max(0, dx):w - max(0, -dx)]
            m = (a >= 0) & (b >= 0)
            ia, ib = a[m], b[m]
            lo.append(np.minimum(ia, ib))
            hi.append(np.maximum(ia, ib))
    if not lo:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(lo), np.concatenate(hi)


def select(xs, ys, w: int, h: int, min_distance: float, max_corners: int, return_rounds: bool = False):
    """the same selection in parallel rounds (what the GPU runs): an undecided candidate is accepted when no undecided or accepted
    candidate with a larger key is in range, dropped when an accepted one is; a decision depends on larger keys only, so the capped
    result is the first max_corners accepted ones in key order"""
    n = len(xs)
    lo, hi = _conflict_pairs(xs, ys, w, h, min_distance)
    state = np.zeros(n, dtype=np.int8)                             # 0 undecided, 1 accepted, 2 dropped
    rounds = []
    while (state == 0).any():
        blocked = np.zeros(n, dtype=bool)
        blocked[hi[state[lo] != 2]] = True                         # a larger key in range that is undecided or accepted
        state[(state == 0) & ~blocked] = 1
        dropped = np.zeros(n, dtype=bool)
        dropped[hi[state[lo] == 1]] = True
        state[(state == 0) & dropped] = 2
        rounds.append(int((state == 0).sum()))
    acc = np.nonzero(state == 1)[0]
    if max_corners > 0:
        acc = acc[:max_corners]
    return (acc, rounds) if return_rounds else acc


def good_features(img, max_corners: int = 3000, quality_level: float = 0.001, min_distance: float = 12.0, order: str = "exact",
                  tie: str = "higher", eig=None):
    """cv::goodFeaturesToTrack: (xy float32 [n, 2], response float32 [n], number of candidates)"""
    if eig is None:
        eig = response(img, order)
    h, w = eig.shape
    xs, ys, v = candidates(eig, quality_level, tie)
    acc = select(xs, ys, w, h, min_distance, max_corners)
    return np.stack([xs[acc], ys[acc]], axis=1).astype(np.float32).reshape(-1, 2), v[acc].astype(np.float32), len(xs)


def fresh(corners_xy, existing_xy, min_distance: float, w: int, h: int) -> np.ndarray:
    """velo.h:132-167 as a rule: a corner is fresh unless an existing point lies at util::dist2 (float arithmetic, compared as double)
    < (float)(min_distance^2); existing points outside [0, w) x [0, h) or non-finite take no part"""
    c = np.asarray(corners_xy, dtype=np.float32).reshape(-1, 2)
    e = np.asarray(existing_xy, dtype=np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(e).all(1) & (e[:, 0] >= 0) & (e[:, 1] >= 0) & (e[:, 0] < f32(w)) & (e[:, 1] < f32(h))
    e = e[ok]
    md2 = np.float64(f32(np.float64(min_distance) * np.float64(min_distance)))
    out = np.ones(len(c), dtype=bool)
    for s in range(0, len(c), 512):
        dx = e[None, :, 0] - c[s:s + 512, None, 0]
        dy = e[None, :, 1] - c[s:s + 512, None, 1]
        d2 = (dx * dx + dy * dy).astype(np.float64)
        out[s:s + 512] = ~(d2 < md2).any(axis=1)
    return out


def detect(img, existing_xy=None, max_corners: int = 3000, quality_level: float = 0.001, min_distance: float = 12.0, eig=None):
    """one velo_detect_job: (xy, response, fresh, counts = [corners, fresh, candidates])"""
    h, w = np.asarray(img).shape
    xy, v, n_cand = good_features(img, max_corners, quality_level, min_distance, eig=eig)
    fr = fresh(xy, np.zeros((0, 2), np.float32) if existing_xy is None else existing_xy, min_distance, w, h)
    return xy, v, fr, np.array([len(xy), int(fr.sum()), n_cand], dtype=np.int32)


# ---- host side of the adaptor: detectFeatures (velo.h:118-177) ---------------------------------------------------------------------

def mat3_apply(M, x, y):
    """Eigen::Matrix3f * (x, y, 1) in float, each row (m0 x + m1 y) + m2, then (p0/p2, p1/p2) (pixel2canonical, velo.h:10-17)"""
    M = np.asarray(M, dtype=np.float32)
    x, y = f32(x), f32(y)
    p = [f32(f32(M[i, 0] * x) + f32(M[i, 1] * y)) + M[i, 2] for i in range(3)]
    return f32(p[0] / p[2]), f32(p[1] / p[2])


def detect_features(img, existing_p, Kinv, id_counter: int, extractor, min_distance: int = 12, **params):
    """velo.h:118-177: detect, extractor(img, keypoints) -> (remaining keypoints, descriptor rows) -- "compute MUTATES cvKP" -- then the
    fresh test over what is left, row kp_i of the descriptors with the kp_i-th remaining keypoint; returns the APPENDED
    (keypoints, keypoints_p, ids, descriptor rows) and the new id_counter"""
    h, w = np.asarray(img).shape
    xy, _, _ = good_features(img, min_distance=float(min_distance), **params)
    left, rows = extractor(img, xy)
    fr = fresh(left, existing_p, float(min_distance), w, h)
    kp, kp_p, ids, desc = [], [], [], []
    for i in np.nonzero(fr)[0]:
        kp_p.append(left[i])
        kp.append(mat3_apply(Kinv, left[i, 0], left[i, 1]))
        desc.append(rows[i])
        ids.append(id_counter)
        id_counter += 1
    return kp, kp_p, ids, np.asarray(desc, np.uint8).reshape(len(ids), -1), id_counter
