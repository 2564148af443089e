"""Numpy restatement of pyramidal Lucas-Kanade tracking as the reference runs it (trackFeatures, velo.h:28-116, on top of
cv::calcOpticalFlowPyrLK) and of consolidateFeatures (velo.h:179-230).  The GPU (velo_set_images / velo_track_features) is held to
this file bit for bit; tests/test_lk_ref.py holds this file to independent sources.

The arithmetic is OpenCV 3.x lkpyramid.cpp as restated in DESIGN.md 2 (unpinned: no OpenCV here), with one deliberate departure:
OpenCV sums the window's A matrix and b vector in float, in SIMD order; this restatement sums them exactly in int64 and rounds once
to float, so the result does not depend on a summation order.  Every float step below is a single IEEE f32 operation (no fusion).

Images are stored per level padded by PAD pixels on every side (PAD >= the largest supported window, 31): the image border is
reflect-101, the derivative border is zero (BORDER_CONSTANT) -- the part of OpenCV's padded pyramid a window of any supported size
can read.
"""
from __future__ import annotations

import numpy as np

PAD = 32                      # border of every stored level (>= max window)
MAX_LEVEL = 7                 # deepest level the library stores / accepts as max_level
MIN_WIN = 5                   # smallest supported window: the stored pyramid is the one this window would build
MAX_WIN = 31
W_BITS = 14
FLT_SCALE = np.float32(1.0 / (1 << 20))
FLT_EPSILON = np.float32(np.finfo(np.float32).eps)
K5 = np.array([1, 4, 6, 4, 1], dtype=np.int64)

f32 = np.float32


def refl101(i, n: int):
    """OpenCV borderInterpolate(BORDER_REFLECT_101) for any offset (folds repeatedly)"""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    period = 2 * (n - 1)
    q = np.mod(i, period)
    return np.where(q >= n, period - q, q)


def pyr_down(img: np.ndarray) -> np.ndarray:
    """cv::pyrDown: [1 4 6 4 1]^T [1 4 6 4 1] / 256 in integers, reflect-101, destination ((w+1)/2, (h+1)/2)"""
    h, w = img.shape
    H, W = (h + 1) // 2, (w + 1) // 2
    ys = refl101(2 * np.arange(H)[:, None] + np.arange(-2, 3)[None, :], h)
    xs = refl101(2 * np.arange(W)[:, None] + np.arange(-2, 3)[None, :], w)
    a = img.astype(np.int64)
    t = (a[:, xs] * K5).sum(-1)                       # (h, W)
    s = (t[ys, :] * K5[None, :, None]).sum(1)         # (H, W)
    return ((s + 128) >> 8).astype(np.uint8)


def scharr(img: np.ndarray):
    """calcSharrDeriv: vertical pass t0 = 3(a+c) + 10b, t1 = c - a; horizontal dx = t0[x+1] - t0[x-1], dy = 3(t1[x+1] + t1[x-1]) + 10 t1[x];
    reflect-101 sampling; int16"""
    h, w = img.shape
    a = img.astype(np.int32)
    yu, yd = refl101(np.arange(h) - 1, h), refl101(np.arange(h) + 1, h)
    t0 = 3 * (a[yu] + a[yd]) + 10 * a
    t1 = a[yd] - a[yu]
    xl, xr = refl101(np.arange(w) - 1, w), refl101(np.arange(w) + 1, w)
    dx = t0[:, xr] - t0[:, xl]
    dy = 3 * (t1[:, xr] + t1[:, xl]) + 10 * t1
    return dx.astype(np.int16), dy.astype(np.int16)


def pad_reflect(img: np.ndarray, p: int = PAD) -> np.ndarray:
    h, w = img.shape
    return img[refl101(np.arange(-p, h + p), h)][:, refl101(np.arange(-p, w + p), w)]


def pad_zero(d: np.ndarray, p: int = PAD) -> np.ndarray:
    out = np.zeros((d.shape[0] + 2 * p, d.shape[1] + 2 * p), dtype=d.dtype)
    out[p:p + d.shape[0], p:p + d.shape[1]] = d
    return out


def level_count(w: int, h: int, win: int, max_level: int) -> int:
    """buildOpticalFlowPyramid's deepest level: after building level l, stop there when l == max_level or the next size
    ((w+1)/2, (h+1)/2) is <= win in either dimension"""
    for lev in range(max_level + 1):
        if lev == max_level:
            return lev
        w, h = (w + 1) // 2, (h + 1) // 2
        if w <= win or h <= win:
            return lev
    return max_level


def build_pyramid(img: np.ndarray):
    """What velo_set_images keeps of one image: levels 0..level_count(w, h, MIN_WIN, MAX_LEVEL), each a dict of the padded image
    (reflect-101), the padded derivatives dx, dy (zero border), the unpadded size and the unpadded level"""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    h, w = img.shape
    L = level_count(w, h, MIN_WIN, MAX_LEVEL)
    out = []
    cur = img
    for lev in range(L + 1):
        if lev > 0:
            cur = pyr_down(cur)
        dx, dy = scharr(cur)
        out.append(dict(img=pad_reflect(cur), dx=pad_zero(dx), dy=pad_zero(dy), w=cur.shape[1], h=cur.shape[0], raw=cur))
    return out


def _weights(a, b):
    one = f32(1.0)
    s = f32(1 << W_BITS)
    iw00 = np.rint(((one - a) * (one - b)) * s).astype(np.int64)
    iw01 = np.rint((a * (one - b)) * s).astype(np.int64)
    iw10 = np.rint(((one - a) * b) * s).astype(np.int64)
    iw11 = (1 << W_BITS) - iw00 - iw01 - iw10
    return iw00, iw01, iw10, iw11


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _bilinear(flat, idx, S, w4):
    iw00, iw01, iw10, iw11 = w4
    return (flat[idx].astype(np.int64) * iw00[:, None] + flat[idx + 1].astype(np.int64) * iw01[:, None] +
            flat[idx + S].astype(np.int64) * iw10[:, None] + flat[idx + S + 1].astype(np.int64) * iw11[:, None])


def _in_bounds(p, win, w, h):
    """floor(p) inside [-win, w) x [-win, h): for integer bounds the same as p inside them, which a NaN coordinate fails (cvFloor of
    NaN gives INT_MIN, outside as well)"""
    return (p[:, 0] >= -win) & (p[:, 0] < w) & (p[:, 1] >= -win) & (p[:, 1] < h)


def _accum(prod, mode):
    if mode == "int64":
        return prod.sum(1).astype(np.float32) * FLT_SCALE
    acc = np.zeros(prod.shape[0], dtype=np.float32)          # OpenCV's scalar path: float, row-major, one pixel at a time
    for k in range(prod.shape[1]):
        acc = acc + prod[:, k].astype(np.float32)
    return acc * FLT_SCALE


def _lane_max(stats, name, prod):
    """stats["lane_max"][name]: the largest |sum| any lane of the GPU's wave holds -- lane l owns window pixels l, l + 64, ... in
    row-major order (velo_track_kernels.h), which is the column order of prod [points, win * win]"""
    if len(prod) == 0:
        return
    n, k = prod.shape
    padded = np.zeros((n, -(-k // 64) * 64), dtype=np.int64)
    padded[:, :k] = prod
    m = int(np.abs(padded.reshape(n, -1, 64).sum(1)).max())
    stats["lane_max"][name] = max(stats["lane_max"].get(name, 0), m)


def track(prev_pyr, next_pyr, pts, win: int = 21, max_level: int = 4, max_count: int = 30, epsilon: float = 0.01,
          min_eig_threshold: float = 1e-4, accumulate: str = "int64", stats=None):
    """calcOpticalFlowPyrLK(prev, next, pts) without initial flow: (next_xy [n,2] f32, status [n] bool).
    accumulate="float": the window sums in float, row-major sequential (OpenCV's scalar order) -- the budget of the unpinned choice.
    stats: optional dict; receives iterations[level] (J samples taken), entered[level] (points that reached the iteration loop) and
    oscillations[level] (points stopped by the |delta + prev_delta| < 0.01 rule).  A stats dict that arrives with a "lane_max" dict
    also receives there, per product (IxIx, IxIy, IyIy, dIx, dIy), the largest |partial sum| of one lane of the GPU's wave over every
    point, level and iteration: what the kernel holds in an int32."""
    pts = np.ascontiguousarray(np.asarray(pts, dtype=np.float32).reshape(-1, 2))
    n = len(pts)
    status = np.ones(n, dtype=bool)
    store = np.zeros((n, 2), dtype=np.float32)
    if n == 0:
        return store, status
    L = min(level_count(prev_pyr[0]["w"], prev_pyr[0]["h"], win, max_level), len(prev_pyr) - 1)
    hw = f32((win - 1) * 0.5)
    eps2 = float(epsilon) * float(epsilon)
    min_eig = f32(min_eig_threshold)
    oy, ox = np.divmod(np.arange(win * win, dtype=np.int64), win)
    if stats is not None:
        stats.setdefault("entered", {})
        stats.setdefault("iterations", {})
        stats.setdefault("oscillations", {})
    for lev in range(L, -1, -1):
        P, Jl = prev_pyr[lev], next_pyr[lev]
        w, h = P["w"], P["h"]
        S = w + 2 * PAD
        prev = pts * f32(1.0 / (1 << lev))
        store = prev.copy() if lev == L else store * f32(2.0)
        pp = prev - hw
        ok = _in_bounds(pp, win, w, h)
        ip = np.floor(np.where(ok[:, None], pp, 0)).astype(np.int64)
        if lev == 0:
            status &= ok
        act = np.nonzero(ok)[0]
        a = pp[act, 0] - ip[act, 0].astype(np.float32)
        b = pp[act, 1] - ip[act, 1].astype(np.float32)
        w4 = _weights(a, b)
        idx = ((ip[act, 1] + PAD) * S + ip[act, 0] + PAD)[:, None] + oy[None, :] * S + ox[None, :]
        Ipatch = _descale(_bilinear(P["img"].reshape(-1), idx, S, w4), W_BITS - 5)
        Ix = _descale(_bilinear(P["dx"].reshape(-1), idx, S, w4), W_BITS)
        Iy = _descale(_bilinear(P["dy"].reshape(-1), idx, S, w4), W_BITS)
        A11, A12, A22 = _accum(Ix * Ix, accumulate), _accum(Ix * Iy, accumulate), _accum(Iy * Iy, accumulate)
        lanes = stats is not None and "lane_max" in stats
        if lanes:
            for name, prod in (("IxIx", Ix * Ix), ("IxIy", Ix * Iy), ("IyIy", Iy * Iy)):
                _lane_max(stats, name, prod)
        D = A11 * A22 - A12 * A12
        minEig = (A22 + A11 - np.sqrt((A11 - A22) * (A11 - A22) + f32(4.0) * A12 * A12)) / f32(2 * win * win)
        bad = (minEig < min_eig) | (D < FLT_EPSILON)
        if lev == 0:
            status[act[bad]] = False
        keep = ~bad
        act, A11, A12, A22, D = act[keep], A11[keep], A12[keep], A22[keep], D[keep]
        Ipatch, Ix, Iy = Ipatch[keep], Ix[keep], Iy[keep]
        Dinv = f32(1.0) / D
        nx = store[act] - hw                                   # running point (top-left corner of the window)
        pdelta = np.zeros((len(act), 2), dtype=np.float32)
        live = np.arange(len(act))                             # rows of `act` still iterating
        if stats is not None:
            stats["entered"][lev] = stats["entered"].get(lev, 0) + len(act)
        Jflat = Jl["img"].reshape(-1)
        for j in range(max_count):
            if len(live) == 0:
                break
            inb = _in_bounds(nx[live], win, w, h)
            if lev == 0:
                status[act[live[~inb]]] = False
            live = live[inb]
            inx = np.floor(nx[live]).astype(np.int64)
            if len(live) == 0:
                break
            if stats is not None:
                stats["iterations"][lev] = stats["iterations"].get(lev, 0) + len(live)
            a = nx[live, 0] - inx[:, 0].astype(np.float32)
            b = nx[live, 1] - inx[:, 1].astype(np.float32)
            jdx = ((inx[:, 1] + PAD) * S + inx[:, 0] + PAD)[:, None] + oy[None, :] * S + ox[None, :]
            diff = _descale(_bilinear(Jflat, jdx, S, _weights(a, b)), W_BITS - 5) - Ipatch[live]
            b1 = _accum(diff * Ix[live], accumulate)
            b2 = _accum(diff * Iy[live], accumulate)
            if lanes:
                _lane_max(stats, "dIx", diff * Ix[live])
                _lane_max(stats, "dIy", diff * Iy[live])
            dlx = (A12[live] * b2 - A22[live] * b1) * Dinv[live]
            dly = (A12[live] * b1 - A11[live] * b2) * Dinv[live]
            nx[live, 0] += dlx
            nx[live, 1] += dly
            st = nx[live] + hw
            conv = (dlx.astype(np.float64) * dlx.astype(np.float64) + dly.astype(np.float64) * dly.astype(np.float64)) <= eps2
            osc = np.zeros(len(live), dtype=bool)
            if j > 0:
                osc = (~conv & (np.abs(dlx + pdelta[live, 0]).astype(np.float64) < 0.01) &
                       (np.abs(dly + pdelta[live, 1]).astype(np.float64) < 0.01))
            if stats is not None:
                stats["oscillations"][lev] = stats["oscillations"].get(lev, 0) + int(osc.sum())
            st[osc, 0] -= dlx[osc] * f32(0.5)
            st[osc, 1] -= dly[osc] * f32(0.5)
            store[act[live]] = st
            pdelta[live, 0] = dlx
            pdelta[live, 1] = dly
            live = live[~(conv | osc)]
    return store, status


def kept(prev_xy, next_xy, status, width: int, height: int, flow_outlier: float = 20000.0):
    """the three filters of trackFeatures (velo.h:72-84): status; util::dist2 (float arithmetic) <= flow_outlier compared as double;
    the point in [0, width) x [0, height)"""
    p = np.asarray(prev_xy, dtype=np.float32).reshape(-1, 2)
    q = np.asarray(next_xy, dtype=np.float32).reshape(-1, 2)
    with np.errstate(invalid="ignore"):                      # non-finite points: their status is 0 already
        dx = p[:, 0] - q[:, 0]
        dy = p[:, 1] - q[:, 1]
        d2 = (dx * dx + dy * dy).astype(np.float64)
    out_of = (q[:, 0] < 0) | (q[:, 1] < 0) | (q[:, 0] >= f32(width)) | (q[:, 1] >= f32(height))
    return np.asarray(status, dtype=bool) & ~(d2 > flow_outlier) & ~out_of


def track_job(prev_pyr, next_pyr, pts, win=21, max_level=4, max_count=30, epsilon=0.01, min_eig_threshold=1e-4, flow_outlier=20000.0):
    """one velo_track_job: (next_xy, status, kept)"""
    nxt, st = track(prev_pyr, next_pyr, pts, win, max_level, max_count, epsilon, min_eig_threshold)
    return nxt, st, kept(pts, nxt, st, prev_pyr[0]["w"], prev_pyr[0]["h"], flow_outlier)


# ---- host side of the adaptor: canonical coordinates and consolidateFeatures (velo.h:10-26, 179-230; utility.h:105-131) ----------

def mat3_apply(M, x, y):
    """Eigen::Matrix3f * (x, y, 1) in float, each row (m0 x + m1 y) + m2, then (p0/p2, p1/p2)"""
    M = np.asarray(M, dtype=np.float32)
    x, y = f32(x), f32(y)
    p = [f32(f32(M[i, 0] * x) + f32(M[i, 1] * y)) + M[i, 2] for i in range(3)]
    return f32(p[0] / p[2]), f32(p[1] / p[2])


GEOMEDIAN_EPS = f32(1e-6)


def _cvnorm(x, y):
    return float(np.sqrt(float(x) * float(x) + float(y) * float(y)))


def geomedian(P):
    """util::geomedian: 20 Weiszfeld iterations in float, cv::norm in double, eps 1e-6"""
    P = [(f32(x), f32(y)) for x, y in P]
    m = len(P)
    yx, yy_ = f32(0.0), f32(0.0)
    for x, y in P:
        yx, yy_ = f32(yx + x), f32(yy_ + y)
    yx, yy_ = f32(yx / f32(m)), f32(yy_ / f32(m))
    for _ in range(20):
        ax, ay, d = f32(0.0), f32(0.0), f32(0.0)
        for x, y in P:
            no = f32(_cvnorm(f32(x - yx), f32(y - yy_)))
            if no < GEOMEDIAN_EPS:
                return yx, yy_
            nn = f32(1.0 / float(no))
            ax, ay = f32(ax + f32(x * nn)), f32(ay + f32(y * nn))
            d = f32(d + nn)
        qx, qy = f32(ax / d), f32(ay / d)
        if _cvnorm(f32(qx - yx), f32(qy - yy_)) < float(GEOMEDIAN_EPS):
            return qx, qy
        yx, yy_ = qx, qy
    return yx, yy_


def consolidate(keypoints, ids, descriptors, K):
    """consolidateFeatures: (keypoints [m,2] f32 canonical, keypoints_p [m,2] f32, ids [m], descriptors [m, cols]) merged per id,
    ids ascending (std::map order); the descriptor of an id is that of its first occurrence"""
    kp = np.asarray(keypoints, dtype=np.float32).reshape(-1, 2)
    desc = np.asarray(descriptors, dtype=np.uint8)
    cols = desc.shape[1] if desc.ndim == 2 else 0
    groups = {}
    for i, k in enumerate(int(v) for v in ids):
        groups.setdefault(k, []).append(i)
    out_kp, out_p, out_ids, out_d = [], [], [], []
    for k in sorted(groups):
        g = groups[k]
        if len(g) > 2:
            gm = geomedian([kp[i] for i in g])
        elif len(g) == 2:
            a, b = kp[g[0]], kp[g[1]]
            gm = (f32(f32(a[0] + b[0]) / f32(2)), f32(f32(a[1] + b[1]) / f32(2)))
        else:
            gm = (kp[g[0], 0], kp[g[0], 1])
        out_ids.append(k)
        out_kp.append(gm)
        out_p.append(mat3_apply(K, gm[0], gm[1]))
        out_d.append(desc[g[0]])
    return (np.asarray(out_kp, dtype=np.float32).reshape(-1, 2), np.asarray(out_p, dtype=np.float32).reshape(-1, 2),
            np.asarray(out_ids, dtype=np.int64), np.asarray(out_d, dtype=np.uint8).reshape(-1, cols))
