"""CPU: the restatements the GPU front end is held to (tests/lk_ref.py, tests/gftt_ref.py, tests/descriptor_ref.py) checked against
independent sources AT THE EDGES of the input and parameter domain (tests/frontend_extremes.py) -- saturated and fastest-texture
images, points on the bounds of the window test, termination parameters at the ends of their ranges, image sizes below one tile,
descriptors at Hamming distance 0 and 512 -- and two integer bounds the kernels rely on, measured: the largest partial sum one lane
of the tracking wave holds (int32) and the largest 3 x 3 box sum of Sobel products (exact in float32 below 2^24)."""
import math

import numpy as np
import pytest

import descriptor_ref as D
import frontend_extremes as X
import gftt_ref as G
import lk_ref as R
import velo_amd  # noqa: F401
from velo_amd import synth
from test_lk_ref import scalar_track

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- 1. the vectorised tracker against the scalar transcription, off the default parameters ----------------------------------------

SCALAR_PARAMS = ([dict(max_count=v) for v in (0, 1, 100)] + [dict(epsilon=v) for v in (0.0, 10.0)] +
                 [dict(min_eig_threshold=v) for v in (0.0, -1.0, 1e3)])


@pytest.mark.parametrize("family", ["noise01", "checker1", "step_edges"])
@pytest.mark.parametrize("win", [5, 9])
def test_track_equals_the_scalar_transcription_off_the_defaults(family, win):
    """96 x 64, the 56 boundary points of the window, one termination parameter at a time: next_xy bit for bit, status equal"""
    w, h = 96, 64
    prev, nxt = X.family_pair(family, w, h, (2, -1))
    P, N = R.build_pyramid(prev), R.build_pyramid(nxt)
    pts = X.boundary_points(w, h, win)
    assert len(pts) <= 60 and np.isfinite(pts).all()
    hw = f32((win - 1) * 0.5)
    for n, col in ((w, 0), (h, 1)):                                  # the set really sits on the bounds of the window test
        c = pts[:, col]
        up = np.nextafter(c, f32(np.inf))
        for b in (f32(-win), f32(n)):
            assert (c - hw == b).any() and ((c - hw < b) & (up - hw >= b)).any(), (n, b)
        assert (c - hw == f32(n - 1)).any()
    tracked = 0
    for params in SCALAR_PARAMS:
        kw = dict(max_count=30, epsilon=0.01, min_eig_threshold=1e-4)
        kw.update(params)
        want_xy, want_st = scalar_track(P, N, pts, win, 2, kw["max_count"], kw["epsilon"], kw["min_eig_threshold"])
        got_xy, got_st = R.track(P, N, pts, win, 2, **kw)
        assert np.array_equal(bits(got_xy), bits(want_xy)), (family, win, params, np.nonzero(bits(got_xy) != bits(want_xy))[0][:8])
        assert np.array_equal(got_st, want_st), (family, win, params)
        if params.get("min_eig_threshold") == 1e3:
            assert not got_st.any()
        tracked += int(got_st.sum())
    if family != "step_edges":
        assert (tracked > 0) == (family == "noise01")                # checker(1) has zero derivatives: nothing tracks


# ---- 2. the int32 bound of a lane's partial sums, measured on the restatement ----------------------------------------------------------

LANE_BOUND = 16 * 8160 * 4080                                       # 16 pixels per lane at window 31, |diff| <= 8160, |Ix| <= 4080


def test_a_lanes_partial_sums_stay_below_2_31_at_window_31():
    """velo_track_kernels.h keeps a lane's share of sum Ix Ix, Ix Iy, Iy Iy, diff Ix and diff Iy in an int (lane l owns window pixels
    l, l + 64, ...; 16 of them at window 31) and argues 16 * 8160 * 4080 = 532,684,800 < 2^31.  Measured here over every point, level
    and iteration on noise01, checker(1) and checker(2) at 641 x 203, 1,056 points: the largest is 332,928,000 = 10 * 8160 * 4080, on
    checker(2) (diff Ix and diff Iy); noise01 reaches 176,637,844; checker(1) has zero central differences, its sums are 0."""
    assert LANE_BOUND < 2 ** 31
    w, h, win = 641, 203, 31
    pts = X.track_points(w, h, win)
    seen = {}
    for family in ("checker1", "noise01", "checker2"):
        st = {"lane_max": {}}
        for shift in X.TRACK_SHIFTS:
            prev, nxt = X.family_pair(family, w, h, shift)
            P, N = R.build_pyramid(prev), R.build_pyramid(nxt)
            for ml in (4, 0):
                R.track(P, N, pts, win, ml, stats=st)
        seen[family] = st["lane_max"]
    worst = max(v for d in seen.values() for v in d.values())
    print(f"largest per-lane |sum| at window 31: {worst} of the argued {LANE_BOUND}; per family {seen}")
    assert worst < 2 ** 31 and worst <= LANE_BOUND, seen
    assert set(seen["noise01"]) == {"IxIx", "IxIy", "IyIy", "dIx", "dIy"} and min(seen["noise01"].values()) > 2 ** 24, seen
    assert max(seen["checker1"].values()) == 0, seen
    assert max(seen["checker2"].values()) > LANE_BOUND // 2, seen    # the measurement comes within a factor 2 of the argued bound


def test_lane_statistics_change_no_result():
    prev, nxt = X.family_pair("noise01", 96, 64, (1, 1))
    P, N = R.build_pyramid(prev), R.build_pyramid(nxt)
    pts = X.uniform_points(50, 96, 64, 1)
    a = R.track(P, N, pts, 9, 2)
    b = R.track(P, N, pts, 9, 2, stats={"lane_max": {}})
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


# ---- 3. the corner restatement at the extremes ---------------------------------------------------------------------------------------

GF_IMAGES = {"noise01": lambda w, h: X.noise01(w, h, 4), "checker1": lambda w, h: X.checker(w, h, 1),
             "checker2": lambda w, h: X.checker(w, h, 2), "stripes2": lambda w, h: X.stripes(w, h, 2)}


@pytest.mark.parametrize("name", list(GF_IMAGES))
def test_gftt_maps_equal_scipy_on_saturated_texture(name):
    nd = pytest.importorskip("scipy.ndimage")
    img = GF_IMAGES[name](67, 45)
    a = img.astype(np.int64)
    kx = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]])
    dx, dy = nd.correlate(a, kx, mode="mirror"), nd.correlate(a, kx.T, mode="mirror")
    gx, gy = G.sobel(img)
    assert np.array_equal(gx, dx) and np.array_equal(gy, dy)
    ones = np.ones((3, 3), np.int64)
    for got, prod in zip(G.box_sums(img), (dx * dx, dx * dy, dy * dy)):
        assert np.array_equal(got, nd.correlate(prod, ones, mode="mirror"))
    eig = G.response(img)
    thr = G.threshold(eig, 0.001)
    e = np.where(eig > thr, eig, f32(0)).astype(np.float32)
    want = (e != 0) & (e == nd.maximum_filter(e, size=3, mode="constant", cval=-np.inf))
    want[0, :] = want[-1, :] = False
    want[:, 0] = want[:, -1] = False
    assert np.array_equal(G.candidate_mask(eig, 0.001), want)
    if name in ("checker1", "stripes2"):
        assert not want.any()                                        # no derivative at all / one direction only: no corner
    else:
        assert want.sum() > 50


BOX_BOUND = 9 * 1020 * 1020


def test_box_sums_stay_below_2_24():
    """gftt_ref.response and the GPU box-sum Sobel products in integers and convert once: exact while |sum| < 2^24.  The analytic
    maximum 9 * 1020^2 = 9,363,600 is REACHED by stripes(2) (|dx| = 1020 on every pixel) and by noise01 at 200 x 120; checker(2)
    gives half of it, 4,681,800; checker(1) 0 (its Sobel derivatives vanish)."""
    assert BOX_BOUND < 2 ** 24
    seen = {}
    for name, make in GF_IMAGES.items():
        seen[name] = int(max(np.abs(s).max() for s in G.box_sums(make(200, 120))))
    print(f"largest |3 x 3 box sum| of Sobel products: {seen} of the analytic {BOX_BOUND}")
    assert max(seen.values()) <= BOX_BOUND < 2 ** 24
    assert seen["stripes2"] == BOX_BOUND and seen["checker1"] == 0 and seen["checker2"] >= BOX_BOUND // 2, seen


@pytest.mark.parametrize("size", X.DETECT_SMALL_SIZES)
def test_gftt_small_sizes_have_no_candidate_without_an_interior_pixel(size):
    w, h = size
    for name, make in GF_IMAGES.items():
        img = make(w, h)
        eig = G.response(img)
        assert eig.shape == (h, w) and np.isfinite(eig).all()
        xy, v, fr, counts = G.detect(img, X.boundary_points(w, h, 5), max_corners=0, min_distance=1.0)
        interior = max(w - 2, 0) * max(h - 2, 0)
        assert counts[2] <= interior and counts[0] == len(xy) == len(v) == len(fr) <= counts[2], (size, name, counts)
        if interior == 0:
            assert counts.tolist() == [0, 0, 0], (size, name)
        xy, v, fr, counts = G.detect(img, None)
        assert counts[0] <= interior


# ---- 4. pyramid and derivatives at sizes below a tile, against explicit index folding ----------------------------------------------

def fold101(i: int, n: int) -> int:
    """reflect-101 by folding at the two ends until the index is inside: -1 -> 1, n -> n - 2"""
    if n == 1:
        return 0
    while i < 0 or i >= n:
        i = -i if i < 0 else 2 * (n - 1) - i
    return i


def slow_pyr_down(img):
    h, w = img.shape
    k = (1, 4, 6, 4, 1)
    out = np.zeros(((h + 1) // 2, (w + 1) // 2), np.uint8)
    for y in range(out.shape[0]):
        for x in range(out.shape[1]):
            s = sum(k[j] * k[i] * int(img[fold101(2 * y + j - 2, h), fold101(2 * x + i - 2, w)]) for j in range(5) for i in range(5))
            out[y, x] = (s + 128) >> 8
    return out


def slow_scharr(img):
    h, w = img.shape
    dx, dy = np.zeros((h, w), np.int16), np.zeros((h, w), np.int16)
    for y in range(h):
        for x in range(w):
            v = [[int(img[fold101(y + j, h), fold101(x + i, w)]) for i in (-1, 0, 1)] for j in (-1, 0, 1)]
            dx[y, x] = 3 * (v[0][2] - v[0][0]) + 10 * (v[1][2] - v[1][0]) + 3 * (v[2][2] - v[2][0])
            dy[y, x] = 3 * (v[2][0] - v[0][0]) + 10 * (v[2][1] - v[0][1]) + 3 * (v[2][2] - v[0][2])
    return dx, dy


def slow_levels(w, h):
    """levels a 5-wide window builds, at most 8: stop when the next size is <= 5 in a dimension"""
    n = 1
    while n < R.MAX_LEVEL + 1 and (w + 1) // 2 > R.MIN_WIN and (h + 1) // 2 > R.MIN_WIN:
        w, h, n = (w + 1) // 2, (h + 1) // 2, n + 1
    return n


@pytest.mark.parametrize("size", X.BUILD_SIZES)
def test_build_pyramid_equals_explicit_folding(size):
    w, h = size
    for img in (X.uniform_noise(w, h, 5), X.noise01(w, h, 6), X.checker(w, h, 1)):
        assert np.array_equal(R.pyr_down(img), slow_pyr_down(img))
        gx, gy = R.scharr(img)
        sx, sy = slow_scharr(img)
        assert np.array_equal(gx, sx) and np.array_equal(gy, sy)
        pyr = R.build_pyramid(img)
        assert len(pyr) == slow_levels(w, h)
        cur = img
        for lev, L in enumerate(pyr):
            if lev:
                cur = slow_pyr_down(cur)
            lh, lw = cur.shape
            assert (L["w"], L["h"]) == (lw, lh) and np.array_equal(L["raw"], cur)
            ys = [fold101(y, lh) for y in range(-R.PAD, lh + R.PAD)]
            xs = [fold101(x, lw) for x in range(-R.PAD, lw + R.PAD)]
            assert np.array_equal(L["img"], cur[np.ix_(ys, xs)])
            sx, sy = slow_scharr(cur)
            for kind, d in (("dx", sx), ("dy", sy)):
                assert np.array_equal(L[kind][R.PAD:R.PAD + lh, R.PAD:R.PAD + lw], d)
                border = L[kind].copy()
                border[R.PAD:R.PAD + lh, R.PAD:R.PAD + lw] = 0
                assert not border.any()


# ---- 5. the matcher restatement on the structured descriptor sets ------------------------------------------------------------------

def slow_match(q, t):
    qi = [int.from_bytes(r.tobytes(), "little") for r in q]
    ti = [int.from_bytes(r.tobytes(), "little") for r in t]
    idx, dist = [], []
    for a in qi:
        best, at = 10 ** 9, -1
        for k, b in enumerate(ti):
            d = bin(a ^ b).count("1")                                # popcount(xor)
            if d < best:
                best, at = d, k
        idx.append(at)
        dist.append(best)
    return np.asarray(idx, np.int32), np.asarray(dist, np.int32)


EXPECTED_DISTANCES = {"zeros_vs_ones": {512}, "ones_vs_zeros": {512}, "zeros_vs_zeros": {0}, "cold_vs_zeros": {511},
                      "exactly_512": {512}, "exactly_511": {511}, "exactly_1": {1}, "hot_vs_cold": {510}, "cold_vs_hot": {510}}


def test_match_restatement_on_structured_descriptors():
    jobs = X.descriptor_jobs()
    assert set(EXPECTED_DISTANCES) <= set(jobs)
    for name, (q, t) in jobs.items():
        idx, dist, md, pairs = D.match(q, t)
        widx, wdist = slow_match(q, t)
        assert np.array_equal(idx, widx) and np.array_equal(dist, wdist), name
        assert md == int(wdist.min())
        keep = ~(wdist.astype(np.float64) > max(1.5 * md, D.MATCH_THRESH))
        assert np.array_equal(pairs, np.stack([np.nonzero(keep)[0], widx[keep]], 1)), name
        if name in EXPECTED_DISTANCES:
            assert set(dist.tolist()) == EXPECTED_DISTANCES[name], (name, set(dist.tolist()))
    rb = X.desc_repeated_bytes()
    _, dist, _, _ = D.match(rb, X.desc_zeros(1))
    assert dist.tolist() == [64 * bin(b).count("1") for b in range(256)]           # every multiple of 64 from 0 to 512


# ---- 6. the leave-out cap of the GPU module, from the restatement alone ----------------------------------------------------------

def test_no_finite_point_can_leave_the_finite_range():
    """The GPU module relaxes bit equality to class equality only on coordinates the restatement reports non-finite.  A step of the
    iteration is (A12 b2 - A22 b1) / D with |A| <= 961 * 4080^2 / 2^20, |b| <= 961 * 8160 * 4080 / 2^20 and D >= FLT_EPSILON: at most
    ~8e15, and the iteration stops once the window has left the level; so a finite point stays finite, and only non-finite INPUT
    points give non-finite results."""
    a = 961 * 4080.0 ** 2 / 2 ** 20
    b = 961 * 8160.0 * 4080.0 / 2 ** 20
    assert 2 * a * b / float(R.FLT_EPSILON) < 1e16 < float(np.finfo(np.float32).max)


@pytest.fixture(scope="module")
def kitti_pair():
    fr = synth.tracking_frames(1226, 370, seed=0)
    return fr["prev"][0], fr["next"][0]


def sweep_reference(prev, nxt, win=21, max_level=4):
    """key -> (next_xy, status, kept) of the restatement for every value of X.SWEEP and the defaults (key None)"""
    h, w = prev.shape
    P, N = R.build_pyramid(prev), R.build_pyramid(nxt)
    pts = X.track_points(w, h, win)
    keys = [None] + [p for p in X.SWEEP if "flow_outlier" not in p]

    def run(p):
        return R.track(P, N, pts, win, max_level, **(p or {}))
    out = {}
    for p, (xy, st) in zip(keys, X.reference_map(run, keys)):
        out[None if p is None else tuple(p.items())[0]] = (xy, st, R.kept(pts, xy, st, w, h))
    xy, st, _ = out[None]
    for p in X.SWEEP:
        if "flow_outlier" in p:
            out[tuple(p.items())[0]] = (xy, st, R.kept(pts, xy, st, w, h, p["flow_outlier"]))
    return pts, out


def check_sweep_is_not_vacuous(pts, out):
    base = out[None]
    for v in (1, 100):
        assert not np.array_equal(bits(out[("max_count", v)][0]), bits(base[0])), v
    assert not out[("min_eig_threshold", 1e3)][1].any()
    moved = (base[0] != pts).any(1)
    assert moved.sum() > 100 and not out[("flow_outlier", 0.0)][2][moved].any()
    assert out[("flow_outlier", 0.0)][2].sum() < base[2].sum() <= out[("flow_outlier", float("inf"))][2].sum()
    assert not out[("flow_outlier", float("-inf"))][2].any()
    assert np.array_equal(out[("max_count", 0)][0], pts) or not np.isfinite(pts).all()


def test_leave_out_shares_of_every_gpu_case(kitti_pair):
    """share of points whose restatement result is non-finite, per GPU tracking case: <= 5 % each, non-zero over the module.  Measured:
    0 in every family and sweep case (see the test above: a finite point stays finite); 4 of 360 = 1.1 % in the step-edge case, the
    four non-finite points of its set."""
    shares = {}
    cases = []
    pyr = {}
    for w, h in X.TRACK_SIZES:
        for name in X.FAMILIES:
            for shift in X.TRACK_SHIFTS:
                prev, nxt = X.family_pair(name, w, h, shift)
                pyr[(name, w, h, shift)] = (R.build_pyramid(prev), R.build_pyramid(nxt))
                cases += [(name, w, h, shift, win, ml) for win, ml in X.TRACK_WINDOWS]

    def run(c):
        name, w, h, shift, win, ml = c
        P, N = pyr[(name, w, h, shift)]
        pts = X.track_points(w, h, win)
        xy, st = R.track(P, N, pts, win, ml)
        assert np.isfinite(xy[np.isfinite(pts).all(1)]).all(), c
        return X.non_finite_share(xy)
    for c, s in zip(cases, X.reference_map(run, cases)):
        shares[c] = s
    for label, (prev, nxt) in (("kitti", kitti_pair), ("noise01", X.family_pair("noise01", 1226, 370, (3, -2)))):
        pts, out = sweep_reference(prev, nxt)
        check_sweep_is_not_vacuous(pts, out)
        for k, (xy, st, kp) in out.items():
            shares[("sweep", label, k)] = X.non_finite_share(xy)
    for w, h in X.TRACK_SIZES:
        prev, nxt = X.family_pair("step_edges", w, h, (3, -2))
        P, N = R.build_pyramid(prev), R.build_pyramid(nxt)
        for win, ml, mineig in ((21, 4, 1e-4), (21, 4, -1.0), (5, 0, 0.0), (31, 2, -1.0)):
            pts = X.step_edge_points(w, h, win)
            xy, st = R.track(P, N, pts, win, ml, min_eig_threshold=mineig)
            fin = np.isfinite(pts).all(1)
            assert np.isfinite(xy[fin]).all() and not st[~fin].any()
            shares[("step_edges", w, h, win, ml, mineig)] = X.non_finite_share(xy)
    worst = max(shares.values())
    nz = {k: v for k, v in shares.items() if v > 0}
    print(f"leave-out shares: {len(shares)} cases, largest {worst:.4f}, non-zero in {len(nz)}: {nz}")
    assert worst <= X.LEAVE_OUT_CAP, nz
    assert len(nz) > 0
