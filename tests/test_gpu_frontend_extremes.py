"""GPU: the visual front end against its restatements (tests/lk_ref.py, tests/gftt_ref.py, tests/descriptor_ref.py) at the edges of
the input and parameter domain (tests/frontend_extremes.py): full-range and saturated images, points on the bounds of the window test
and far outside, every termination parameter of Lucas-Kanade at the ends of its range (single and batch entry), image sizes from
1 x 1 to 16384 x 1, detection with no interior pixel and with tens of thousands of corners, descriptors at Hamming distance 0, 1, 511
and 512.  Comparators as in test_gpu_track / test_gpu_detect / test_gpu_match: next_xy and responses FLOAT-BIT-EQUAL, the rest
ARRAY-EQUAL.  The one relaxation: where the restatement's next_xy is non-finite, the NaN / +inf / -inf class per coordinate is
compared instead of the bits; the share of such points is at most 5 % per case (tests/test_frontend_extremes_cpu.py computes it from
the restatement alone), non-zero in the step-edge cases (their four non-finite points), and status and kept are compared for every
point."""
import os

import numpy as np
import pytest

import descriptor_ref as D
import frontend_extremes as X
import gftt_ref as G
import lk_ref as R
import velo_amd  # noqa: F401
from velo_amd import api, synth

pytestmark = pytest.mark.gpu

LEFT_OUT = {}                                   # case -> share of points compared by class only


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def check_track(case, got, want):
    """got / want: (next_xy, status, kept) of one job"""
    gxy, wxy = np.asarray(got[0], np.float32), np.asarray(want[0], np.float32)
    fin = np.isfinite(wxy)
    share = X.non_finite_share(wxy)
    LEFT_OUT[case] = share
    assert share <= X.LEAVE_OUT_CAP, (case, share)
    bad = bits(gxy)[fin] != bits(wxy)[fin]
    assert not bad.any(), (case, int(bad.sum()), np.argwhere(bits(gxy) != bits(wxy))[:8].tolist())
    assert np.array_equal(np.isnan(gxy), np.isnan(wxy)), case
    assert np.array_equal(np.isposinf(gxy), np.isposinf(wxy)) and np.array_equal(np.isneginf(gxy), np.isneginf(wxy)), case
    assert np.array_equal(got[1], want[1]), (case, np.nonzero(got[1] != want[1])[0][:8])
    assert np.array_equal(got[2], want[2]), (case, np.nonzero(got[2] != want[2])[0][:8])


# ---- tracking: every image family ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", X.TRACK_SIZES)
@pytest.mark.parametrize("family", list(X.FAMILIES))
def test_track_every_family(hip_lib, family, size):
    w, h = size
    for shift in X.TRACK_SHIFTS:
        prev, nxt = X.family_pair(family, w, h, shift)
        P, N = R.build_pyramid(prev), R.build_pyramid(nxt)
        want = X.reference_map(lambda wm: R.track_job(P, N, X.track_points(w, h, wm[0]), win=wm[0], max_level=wm[1]), X.TRACK_WINDOWS)
        c = api.Context(0)
        try:
            c.set_images([prev])
            c.set_images([nxt])
            for (win, ml), ref in zip(X.TRACK_WINDOWS, want):
                got = c.track_features([(0, 0, X.track_points(w, h, win))], window=win, max_level=ml)
                check_track((family, size, shift, win, ml), (got[0][0], got[1][0], got[2][0]), ref)
        finally:
            c.close()
        if family in ("noise01", "uniform_noise") and shift == (3, -2):
            xy, st, _ = want[1]                                        # window 21, all levels: most points find the known motion
            pts = X.track_points(w, h, 21)[:X.N_UNIFORM]
            inner = (np.abs(pts - np.array([w / 2, h / 2])) < np.array([w / 2 - 40, h / 2 - 40])).all(1) & st[:X.N_UNIFORM]
            assert (np.abs(xy[:X.N_UNIFORM] - pts - np.array(shift, np.float32)).max(1) < 0.5)[inner].mean() > 0.5
        if family.startswith("saturated") or family == "checker1":
            assert not any(ref[1].any() for ref in want)               # no derivative anywhere: every point loses its status


# ---- tracking: the termination parameters, one at a time -------------------------------------------------------------------------

def sweep_key(p):
    return None if p is None else tuple(p.items())[0]


def sweep_reference(P, N, pts, w, h, win=21, max_level=4):
    keys = [None] + [p for p in X.SWEEP if "flow_outlier" not in p]
    out = {}
    for p, (xy, st) in zip(keys, X.reference_map(lambda p: R.track(P, N, pts, win, max_level, **(p or {})), keys)):
        out[sweep_key(p)] = (xy, st, R.kept(pts, xy, st, w, h))
    xy, st, _ = out[None]
    for p in X.SWEEP:
        if "flow_outlier" in p:
            out[sweep_key(p)] = (xy, st, R.kept(pts, xy, st, w, h, p["flow_outlier"]))
    return out


def check_sweep_is_not_vacuous(pts, res):
    base = res[None]
    for v in (1, 100):
        assert (bits(res[("max_count", v)][0]) != bits(base[0])).any(), v
    assert not res[("min_eig_threshold", 1e3)][1].any() and not res[("min_eig_threshold", 1e3)][2].any()
    moved = (base[0] != pts).any(1)
    assert moved.sum() > 100 and not res[("flow_outlier", 0.0)][2][moved].any()
    assert not res[("flow_outlier", float("-inf"))][2].any()
    assert res[("flow_outlier", float("inf"))][2].sum() >= base[2].sum() > res[("flow_outlier", 0.0)][2].sum()


def sweep_images(label):
    if label == "kitti":
        fr = synth.tracking_frames(1226, 370, seed=0)
        return fr["prev"][0], fr["next"][0]
    return X.family_pair("noise01", 1226, 370, (3, -2))


@pytest.mark.parametrize("label", ["kitti", "noise01"])
def test_track_parameter_sweep(hip_lib, label):
    prev, nxt = sweep_images(label)
    h, w = prev.shape
    P, N = R.build_pyramid(prev), R.build_pyramid(nxt)
    pts = X.track_points(w, h, 21)
    want = sweep_reference(P, N, pts, w, h)
    c = api.Context(0)
    got = {}
    try:
        c.set_images([prev])
        c.set_images([nxt])
        for p in [None] + X.SWEEP:
            g = c.track_features([(0, 0, pts)], **(p or {}))
            got[sweep_key(p)] = (g[0][0], g[1][0], g[2][0])
    finally:
        c.close()
    for k in want:
        check_track(("sweep", label, k), got[k], want[k])
    check_sweep_is_not_vacuous(pts, got)
    assert np.array_equal(bits(got[("max_count", 0)][0][:X.N_UNIFORM]), bits(pts[:X.N_UNIFORM]))     # no iteration: the point itself


def test_track_parameter_sweep_batch_equals_single_calls(hip_lib):
    """three contexts of different sizes, two cameras in one: every sweep value through velo_track_features_batch gives the bytes of
    the single calls"""
    kp, kn = sweep_images("kitti")
    n0, n1 = X.family_pair("noise01", 641, 203, (3, -2))
    e0, e1 = X.family_pair("step_edges", 320, 160, (3, -2))
    pairs = [([kp, X.shifted(kp, 2, 1)], [kn, X.shifted(kn, 2, 1)]), ([n0, n0], [n1, n1]), ([e0, e0], [e1, e1])]   # (previous, current)
    sizes = [(1226, 370), (641, 203), (320, 160)]
    pts = [np.concatenate([X.track_points(w, h, 21)[500:], X.NON_FINITE_POINTS]) for w, h in sizes]
    ctxs = [api.Context(0) for _ in sizes]
    try:
        api.set_images_batch(ctxs, [p[0] for p in pairs])
        api.set_images_batch(ctxs, [p[1] for p in pairs])
        jobs = [(0, 0, 0, pts[0]), (1, 0, 1, pts[1]), (2, 1, 1, pts[2]), (0, 1, 0, pts[0][:65]), (1, 1, 0, pts[1][:0]), (2, 0, 0, pts[2][:1])]
        differs = 0
        base = None
        for p in [None] + X.SWEEP:
            kw = p or {}
            got = api.track_features_batch(ctxs, jobs, **kw)
            for j, (ci, pc, cc, xy) in enumerate(jobs):
                one = ctxs[ci].track_features([(pc, cc, xy)], **kw)
                for a, b in zip(one, got):
                    assert a[0].tobytes() == b[j].tobytes(), (p, j)
            if p is None:
                base = got
            else:
                differs += any(a.tobytes() != b.tobytes() for ga, gb in zip(got, base) for a, b in zip(ga, gb))
        assert differs >= 10                                             # the values are not ignored by the batch entry
    finally:
        for c in ctxs:
            c.close()


# ---- tracking: divergent iterations on edges -------------------------------------------------------------------------------------

@pytest.mark.parametrize("size", X.TRACK_SIZES)
def test_track_step_edges_divergent_iterations(hip_lib, size):
    """points on straight 0 | 255 edges (one gradient direction in the window) with the minimum-eigenvalue test at its default and
    switched off (threshold -1 or 0), so that only the D < FLT_EPSILON test stands between the edge and the division; plus four
    non-finite points, the only way to a non-finite result (tests/test_frontend_extremes_cpu.py)"""
    w, h = size
    prev, nxt = X.family_pair("step_edges", w, h, (3, -2))
    P, N = R.build_pyramid(prev), R.build_pyramid(nxt)
    c = api.Context(0)
    try:
        c.set_images([prev])
        c.set_images([nxt])
        for win, ml, mineig in ((21, 4, 1e-4), (21, 4, -1.0), (5, 0, 0.0), (31, 2, -1.0)):
            pts = X.step_edge_points(w, h, win)
            want = R.track_job(P, N, pts, win=win, max_level=ml, min_eig_threshold=mineig)
            got = c.track_features([(0, 0, pts)], window=win, max_level=ml, min_eig_threshold=mineig)
            check_track(("step_edges", w, h, win, ml, mineig), (got[0][0], got[1][0], got[2][0]), want)
            assert LEFT_OUT[("step_edges", w, h, win, ml, mineig)] > 0
    finally:
        c.close()


# ---- image build at small and degenerate sizes -----------------------------------------------------------------------------------

@pytest.mark.parametrize("n_cams", [1, 3])
@pytest.mark.parametrize("size", X.BUILD_SIZES_GPU)
def test_build_and_track_small_sizes(hip_lib, size, n_cams):
    w, h = size
    prev = [X.uniform_noise(w, h, 20 + k) for k in range(n_cams)]
    nxt = [X.shifted(im, 1, 0) if w > 1 else X.shifted(im, 0, 1) for im in prev]
    P, N = [R.build_pyramid(i) for i in prev], [R.build_pyramid(i) for i in nxt]
    c = api.Context(0)
    try:
        c.set_images(prev)
        c.set_images(nxt)
        for previous, pyrs in ((True, P), (False, N)):
            assert c.image_levels(previous=previous) == len(pyrs[0])
            for cam in range(n_cams):
                for lev, L in enumerate(pyrs[cam]):
                    for kind in ("img", "dx", "dy"):
                        got, pad = c.get_image_level(cam, lev, kind, previous=previous)
                        assert pad == R.PAD and got.shape == L[kind].shape
                        assert np.array_equal(got, L[kind]), (size, n_cams, previous, cam, lev, kind)
        pts = np.concatenate([X.boundary_points(w, h, 5), X.uniform_points(40, w, h, 9)])
        jobs = [(k, (k + 1) % n_cams, pts) for k in range(n_cams)]
        got = c.track_features(jobs, window=5)
        for j, (pc, cc, xy) in enumerate(jobs):
            check_track(("small", size, n_cams, j), (got[0][j], got[1][j], got[2][j]), R.track_job(P[pc], N[cc], xy, win=5))
    finally:
        c.close()


# ---- detection -----------------------------------------------------------------------------------------------------------------------

DETECT_IMAGES = {"noise01": lambda w, h: X.noise01(w, h, 4), "uniform_noise": lambda w, h: X.uniform_noise(w, h, 5),
                 "checker1": lambda w, h: X.checker(w, h, 1), "checker2": lambda w, h: X.checker(w, h, 2),
                 "saturated0": lambda w, h: X.saturated(w, h, 0), "saturated255": lambda w, h: X.saturated(w, h, 255),
                 "stripes2": lambda w, h: X.stripes(w, h, 2)}
DETECT_PARAMS = (dict(), dict(max_corners=0, min_distance=1.0))


def detect_expected(img, existing, params, eig):
    """gftt_ref.detect; above 100,000 candidates with a minimum distance (checker(2): 447,252 equal responses) the selection is the
    literal loop of featureselect.cpp, gftt_ref.select_scalar, which stops at the cap -- the parallel-round form (held to it by
    tests/test_gftt_ref.py) would list ~1e8 conflicting pairs"""
    mc, md = params.get("max_corners", 3000), params.get("min_distance", 12.0)
    h, w = img.shape
    xs, ys, v = G.candidates(eig, 0.001)
    if len(xs) <= 100000 or md <= 1.0:
        return G.detect(img, existing, mc, 0.001, md, eig=eig)
    acc = G.select_scalar(xs, ys, w, h, md, mc)
    xy = np.stack([xs[acc], ys[acc]], axis=1).astype(np.float32).reshape(-1, 2)
    fr = G.fresh(xy, np.zeros((0, 2), np.float32) if existing is None else existing, md, w, h)
    return xy, v[acc].astype(np.float32), fr, np.array([len(xy), int(fr.sum()), len(xs)], dtype=np.int32)


def check_detect(got, counts, want, tag):
    xy, v, fr, cn = want
    assert counts.tolist() == cn.tolist(), (tag, counts, cn)
    assert np.array_equal(got[0], xy) and np.array_equal(bits(got[1]), bits(v)) and np.array_equal(got[2], fr), tag


@pytest.mark.parametrize("size", ((1226, 370),) + X.DETECT_SMALL_SIZES)
def test_detect_extreme_images_and_sizes(hip_lib, size):
    """the seven images are the seven cameras of one context"""
    w, h = size
    names = list(DETECT_IMAGES)
    imgs = [DETECT_IMAGES[n](w, h) for n in names]
    eigs = [G.response(i) for i in imgs]
    ex = np.concatenate([X.boundary_points(w, h, 5), X.uniform_points(300, w, h, 13), X.NON_FINITE_POINTS])
    jobs = [(cam, ex if cam % 2 == 0 else None) for cam in range(len(imgs))]
    want = {i: X.reference_map(lambda j: detect_expected(imgs[j[0]], j[1], p, eigs[j[0]]), jobs) for i, p in enumerate(DETECT_PARAMS)}
    c = api.Context(0)
    try:
        c.set_images(imgs)
        for cam in range(len(imgs)):
            got = c.corner_response(cam)
            d = bits(got) != bits(eigs[cam])
            assert got.shape == (h, w) and not d.any(), (size, names[cam], int(d.sum()), np.argwhere(d)[:8].tolist())
        for i, p in enumerate(DETECT_PARAMS):
            got, counts = c.detect_features(jobs, return_counts=True, **p)
            for j in range(len(jobs)):
                check_detect(got[j], counts[j], want[i][j], (size, names[j], p))
            if max(w - 2, 0) * max(h - 2, 0) == 0:
                assert not counts.any()
        if size == (1226, 370):
            n01 = want[1][names.index("noise01")][3]
            assert n01[0] == n01[2] > 20000                            # every candidate a corner: above 4096, the capacity retry and the global sort
            assert all(want[1][names.index(n)][3][0] == 0 for n in ("checker1", "saturated0", "saturated255", "stripes2"))
    finally:
        c.close()


def test_detect_batch_mixes_3x3_17x3_and_full_size(hip_lib):
    sizes = [(3, 3), (17, 3), (1226, 370)]
    imgs = [[X.noise01(w, h, 30 + k), X.uniform_noise(w, h, 40 + k)] for k, (w, h) in enumerate(sizes)]
    ex = [np.concatenate([X.boundary_points(w, h, 5), X.uniform_points(200, w, h, 3)]) for w, h in sizes]
    ctxs = [api.Context(0) for _ in sizes]
    try:
        api.set_images_batch(ctxs, imgs)
        jobs = [(0, 0, ex[0]), (2, 1, ex[2]), (1, 0, None), (1, 1, ex[1]), (0, 1, None), (2, 0, None)]
        for p in DETECT_PARAMS:
            got, counts = api.detect_features_batch(ctxs, jobs, return_counts=True, **p)
            for j, (ci, cam, e) in enumerate(jobs):
                one, cn = ctxs[ci].detect_features([(cam, e)], return_counts=True, **p)
                assert counts[j].tolist() == cn[0].tolist(), (p, j)
                for a, b in zip(one[0], got[j]):
                    assert a.tobytes() == b.tobytes(), (p, j)
                check_detect(got[j], counts[j], detect_expected(imgs[ci][cam], e, p, G.response(imgs[ci][cam])), (p, j))
    finally:
        for c in ctxs:
            c.close()


# ---- matching ----------------------------------------------------------------------------------------------------------------------

def check_match(got, want, tag):
    for a, b in zip(got[:2], want[:2]):
        assert np.array_equal(a, b), tag
    assert int(got[2]) == int(want[2]) and np.array_equal(got[3], want[3]), tag


def test_match_structured_descriptors(hip_lib, diag_lib):
    jobs = X.descriptor_jobs()
    names = list(jobs)
    want = {n: D.match(*jobs[n]) for n in names}
    seen = set()
    for n in names:
        seen |= set(want[n][1].tolist())
    assert {0, 1, 510, 511, 512} <= seen                                 # both ends of the distance range are in the expected output
    assert want["zeros_vs_ones"][2] == 512 and want["exactly_512"][2] == 512 and want["exactly_511"][2] == 511 and want["exactly_1"][2] == 1
    os.environ["VELO_MATCH_VARIANT"] = "0"
    try:
        dctx = api.Context(0, lib=diag_lib)
    finally:
        del os.environ["VELO_MATCH_VARIANT"]
    c = api.Context(0)
    try:
        for n in names:
            check_match(c.match_descriptors(*jobs[n]), want[n], n)
        assert c.match_descriptors(*jobs["zeros_vs_ones"])[2] == 512
        batch = [jobs[n] for n in names]
        for ctx, tag in ((c, "product"), (dctx, "xor variant")):
            idx, dist, md, pairs = ctx.match_descriptor_jobs(batch)
            for j, n in enumerate(names):
                check_match((idx[j], dist[j], md[j], pairs[j]), want[n], (tag, n))
    finally:
        c.close()
        dctx.close()
