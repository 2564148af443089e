"""CPU: the Lucas-Kanade restatement (tests/lk_ref.py) held to independent sources -- pyrDown and Scharr against
scipy.ndimage.correlate (mode "mirror" is reflect-101), the vectorised tracker against a literal scalar transcription of the per-point
loop, ground-truth motion on rendered frames, consolidation against hand-computed cases, and the budget of the unpinned choice
(float accumulation against exact int64 sums).  Also: the C entry points refuse bad arguments before they touch a device."""
import ctypes as C
import math

import numpy as np
import pytest

import lk_ref as R
import velo_amd  # noqa: F401
from velo_amd import api, build, synth

f32 = np.float32


# ---- pyramid and derivatives ------------------------------------------------------------------------------------------------------

def test_pyr_down_and_scharr_equal_scipy_correlate():
    nd = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(0)
    for h, w in ((370, 1226), (203, 641), (7, 9), (2, 3), (1, 5), (6, 1)):
        img = rng.integers(0, 256, (h, w), dtype=np.uint8)
        k5 = np.outer([1, 4, 6, 4, 1], [1, 4, 6, 4, 1])
        full = nd.correlate(img.astype(np.int64), k5, mode="mirror")
        want = ((full[::2, ::2] + 128) >> 8).astype(np.uint8)
        assert want.shape == ((h + 1) // 2, (w + 1) // 2)
        if min(h, w) >= 3:                                  # scipy's mirror and OpenCV's reflect-101 agree while the offset is < n
            assert np.array_equal(R.pyr_down(img), want), (h, w)
        kx = np.array([[-3, 0, 3], [-10, 0, 10], [-3, 0, 3]])
        dx = nd.correlate(img.astype(np.int64), kx, mode="mirror")
        dy = nd.correlate(img.astype(np.int64), kx.T, mode="mirror")
        gx, gy = R.scharr(img)
        if min(h, w) >= 2:
            assert np.array_equal(gx, dx) and np.array_equal(gy, dy), (h, w)


def test_reflect101_folds_and_pad():
    assert R.refl101(np.arange(-5, 9), 4).tolist() == [1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2]
    assert R.refl101([-3, 0, 7], 1).tolist() == [0, 0, 0]
    img = np.arange(12, dtype=np.uint8).reshape(3, 4)
    p = R.pad_reflect(img, 2)
    assert p[2:5, 2:6].tolist() == img.tolist() and p[0, 2:6].tolist() == img[2].tolist() and p[2, 0] == img[0, 2]


def test_level_counts():
    assert R.level_count(1226, 370, 21, 4) == 4                  # the issue's KITTI case: all 5 levels
    assert len(R.build_pyramid(np.zeros((370, 1226), np.uint8))) == 7
    assert R.level_count(100, 40, 21, 4) == 0                    # next height 20 <= 21
    assert R.level_count(100, 50, 21, 4) == 1


# ---- the tracker: a literal scalar transcription of LKTrackerInvoker, point by point --------------------------------------------

def _floor(v):
    """cvFloor: a NaN or infinite coordinate converts to INT_MIN (the x86 'integer indefinite' value), which fails every bounds test"""
    v = float(v)
    return int(math.floor(v)) if math.isfinite(v) else -2 ** 31


def scalar_track(prev_pyr, next_pyr, pts, win, max_level, max_count=30, epsilon=0.01, min_eig=1e-4):
    L = min(R.level_count(prev_pyr[0]["w"], prev_pyr[0]["h"], win, max_level), len(prev_pyr) - 1)
    hw = f32((win - 1) * 0.5)
    out, sts = [], []
    for x0, y0 in np.asarray(pts, np.float32):
        status = True
        nxt = (f32(0), f32(0))
        for lev in range(L, -1, -1):
            P, J = prev_pyr[lev], next_pyr[lev]
            w, h, S = P["w"], P["h"], P["w"] + 2 * R.PAD
            I, DX, DY, JJ = P["img"], P["dx"], P["dy"], J["img"]
            sc = f32(1.0 / (1 << lev))
            prev = (f32(x0 * sc), f32(y0 * sc))
            nxt = prev if lev == L else (f32(nxt[0] * f32(2)), f32(nxt[1] * f32(2)))
            px, py = f32(prev[0] - hw), f32(prev[1] - hw)
            ix, iy = _floor(px), _floor(py)
            if ix < -win or ix >= w or iy < -win or iy >= h:
                if lev == 0:
                    status = False
                continue
            w4 = [int(v[0]) for v in R._weights(np.array([f32(px - f32(ix))]), np.array([f32(py - f32(iy))]))]

            def samp(img, x, y):
                X, Y = x + R.PAD, y + R.PAD
                return (int(img[Y, X]) * w4[0] + int(img[Y, X + 1]) * w4[1] + int(img[Y + 1, X]) * w4[2] + int(img[Y + 1, X + 1]) * w4[3])
            Iw, Ixw, Iyw = [], [], []
            a11 = a12 = a22 = 0
            for yy in range(win):
                for xx in range(win):
                    Iw.append((samp(I, ix + xx, iy + yy) + 256) >> 9)
                    gx = (samp(DX, ix + xx, iy + yy) + 8192) >> 14
                    gy = (samp(DY, ix + xx, iy + yy) + 8192) >> 14
                    Ixw.append(gx)
                    Iyw.append(gy)
                    a11 += gx * gx
                    a12 += gx * gy
                    a22 += gy * gy
            A11, A12, A22 = (f32(f32(a11) * R.FLT_SCALE), f32(f32(a12) * R.FLT_SCALE), f32(f32(a22) * R.FLT_SCALE))
            D = f32(f32(A11 * A22) - f32(A12 * A12))
            t = f32(f32(f32(A11 - A22) * f32(A11 - A22)) + f32(f32(f32(4) * A12) * A12))
            me = f32(f32(f32(A22 + A11) - f32(np.sqrt(t))) / f32(2 * win * win))
            if me < f32(min_eig) or D < R.FLT_EPSILON:
                if lev == 0:
                    status = False
                continue
            Dinv = f32(f32(1) / D)
            nx, ny = f32(nxt[0] - hw), f32(nxt[1] - hw)
            pd = (f32(0), f32(0))
            for j in range(max_count):
                jx, jy = _floor(nx), _floor(ny)
                if jx < -win or jx >= w or jy < -win or jy >= h:
                    if lev == 0:
                        status = False
                    break
                w4 = [int(v[0]) for v in R._weights(np.array([f32(nx - f32(jx))]), np.array([f32(ny - f32(jy))]))]
                b1 = b2 = 0
                k = 0
                for yy in range(win):
                    for xx in range(win):
                        diff = ((samp(JJ, jx + xx, jy + yy) + 256) >> 9) - Iw[k]
                        b1 += diff * Ixw[k]
                        b2 += diff * Iyw[k]
                        k += 1
                B1, B2 = f32(f32(b1) * R.FLT_SCALE), f32(f32(b2) * R.FLT_SCALE)
                dx = f32(f32(f32(A12 * B2) - f32(A22 * B1)) * Dinv)
                dy = f32(f32(f32(A12 * B1) - f32(A11 * B2)) * Dinv)
                nx, ny = f32(nx + dx), f32(ny + dy)
                nxt = (f32(nx + hw), f32(ny + hw))
                if float(dx) * float(dx) + float(dy) * float(dy) <= epsilon * epsilon:
                    break
                if j > 0 and abs(float(f32(dx + pd[0]))) < 0.01 and abs(float(f32(dy + pd[1]))) < 0.01:
                    nxt = (f32(nxt[0] - f32(dx * f32(0.5))), f32(nxt[1] - f32(dy * f32(0.5))))
                    break
                pd = (dx, dy)
        out.append(nxt)
        sts.append(status)
    return np.asarray(out, np.float32).reshape(-1, 2), np.asarray(sts, bool)


@pytest.fixture(scope="module")
def small_frames():
    fr = synth.tracking_frames(160, 96, seed=2, motion=dict(tx=1.7, ty=-0.9, angle=0.01, scale=1.01), flat=True)
    return fr, [R.build_pyramid(i) for i in fr["prev"]], [R.build_pyramid(i) for i in fr["next"]]


def test_vectorised_equals_scalar_transcription_bit_for_bit(small_frames):
    """201 points: interior, borders, outside the image, inside the flat patches, NaN and infinite coordinates; windows 7 and 9.
    The set exercises the oscillation rule (|delta + prev_delta| < 0.01 in both coordinates: stop at next - delta / 2)."""
    fr, P, N = small_frames
    rng = np.random.default_rng(1)
    pts = [synth.tracking_points(180, 160, 96, seed=8, margin=-12.0),
           np.array([[0, 0], [159.9, 95.9], [-3.5, 40], [170, 50], [80, -20], [0.5, 95.5], [np.nan, 30], [40, np.inf],
                     [-np.inf, 10]], np.float32)]
    for x0, y0, x1, y1 in fr["flat"]:                               # inside the flat rectangles: minimum-eigenvalue rejection
        pts.append(np.stack([rng.uniform(x0 + 12, x1 - 12, 6), rng.uniform(y0 + 12, y1 - 12, 6)], 1).astype(np.float32))
    pts = np.concatenate(pts)
    assert len(pts) == 201
    for win, ml, cam in ((7, 3, 0), (9, 2, 1)):
        want_xy, want_st = scalar_track(P[0], N[cam], pts, win, ml)
        st = {}
        got_xy, got_st = R.track(P[0], N[cam], pts, win, ml, stats=st)
        fin = np.isfinite(pts).all(1)
        assert np.array_equal(got_xy[fin].view(np.uint32), want_xy[fin].view(np.uint32))
        assert np.array_equal(np.isnan(got_xy), np.isnan(want_xy))
        assert np.array_equal(got_st, want_st)
        assert 0 < want_st.sum() < len(pts) and not want_st[~fin].any()
        assert st["oscillations"][0] > 0 and sum(st["oscillations"].values()) > 10, st["oscillations"]


def test_flat_patches_fail_the_min_eigenvalue_test(small_frames):
    fr, P, N = small_frames
    x0, y0, x1, y1 = fr["flat"][0]
    c = np.array([[0.5 * (x0 + x1), 0.5 * (y0 + y1)]], np.float32)
    _, st = R.track(P[0], N[0], c, win=7, max_level=0)
    assert not st[0]


def test_recovers_true_motion_on_rendered_frames():
    """textured interior points of both cameras; threshold set from what the restatement achieves (median 0.02-0.03 px, 95th
    percentile 0.05 px on this scene): median <= 0.05 px, 95 % <= 0.15 px"""
    fr = synth.tracking_frames(1226, 370, seed=0)
    P = [R.build_pyramid(i) for i in fr["prev"]]
    N = [R.build_pyramid(i) for i in fr["next"]]
    pts = synth.tracking_points(1500, seed=5, margin=40.0)
    m = fr["motion"]
    d = np.array([synth.LK_DISPARITY, 0.0])
    for cam in range(2):
        nxt, st = R.track(P[cam], N[cam], pts)
        shift = d if cam == 1 else 0.0                             # camera 1 sees the scene point p at p - d
        truth = synth.texture_motion(pts + shift, 1226, 370, m["tx"], m["ty"], m["angle"], m["scale"]) - shift
        flat = np.zeros(len(pts), bool)
        for x0, y0, x1, y1 in fr["flat"]:
            flat |= (pts[:, 0] > x0 - 25) & (pts[:, 0] < x1 + 25) & (pts[:, 1] > y0 - 25) & (pts[:, 1] < y1 + 25)
        ok = st & ~flat
        assert ok.sum() > 0.9 * (~flat).sum()
        err = np.linalg.norm(nxt[ok] - truth[ok], axis=1)
        assert np.median(err) <= 0.05 and np.percentile(err, 95) <= 0.15, (np.median(err), np.percentile(err, 95))
    # the stereo pair: camera 0's points tracked into camera 1 of the next frame move by the motion plus the disparity
    nxt, st = R.track(P[0], N[1], pts)
    truth = synth.texture_motion(pts, 1226, 370, m["tx"] - synth.LK_DISPARITY, m["ty"], m["angle"], m["scale"])
    err = np.linalg.norm(nxt[st] - truth[st], axis=1)
    assert np.median(err) <= 0.05


def test_kept_filter():
    prev = np.array([[10, 10], [10, 10], [10, 10], [0, 0], [5, 5]], np.float32)
    nxt = np.array([[11, 12], [-0.001, 3], [10, 100], [200, 0], [5, 5]], np.float32)
    st = np.array([1, 1, 1, 1, 0], bool)
    assert R.kept(prev, nxt, st, 100, 50, flow_outlier=20000).tolist() == [True, False, False, False, False]
    assert R.kept(prev, nxt, st, 300, 150, flow_outlier=20000).tolist() == [True, False, True, False, False]
    assert R.kept(prev, nxt, st, 300, 150, flow_outlier=40000).tolist() == [True, False, True, True, False]      # 40000 is not > 40000


# ---- consolidation (velo.h:179-230) -----------------------------------------------------------------------------------------------

K = np.array([[718.856, 0, 607.1928], [0, 718.856, 185.2157], [0, 0, 1]], np.float32)


def test_consolidate_pairs_singles_and_id_order():
    kp = np.array([[0.1, 0.2], [0.3, -0.1], [0.5, 0.6], [0.2, 0.2]], np.float32)
    desc = np.arange(4 * 3, dtype=np.uint8).reshape(4, 3)
    out_kp, out_p, ids, d = R.consolidate(kp, [7, 3, 7, 1], desc, K)
    assert ids.tolist() == [1, 3, 7]                               # std::map order
    assert np.array_equal(out_kp[0], kp[3]) and np.array_equal(out_kp[1], kp[1])
    assert out_kp[2].tolist() == [f32(f32(f32(0.1) + f32(0.5)) / f32(2)), f32(f32(f32(0.2) + f32(0.6)) / f32(2))]
    assert d.tolist() == [desc[3].tolist(), desc[1].tolist(), desc[0].tolist()]     # the first occurrence's row
    x = f32(f32(f32(K[0, 0] * out_kp[2, 0]) + f32(K[0, 1] * out_kp[2, 1])) + K[0, 2])
    assert out_p[2, 0] == x                                        # K * (x, y, 1), z = 1
    assert abs(float(out_p[1, 1]) - (718.856 * -0.1 + 185.2157)) < 1e-3


def test_consolidate_geomedian_cases():
    # three points: the Weiszfeld iteration, against an independent double-precision solution
    pts = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]], np.float32)
    gm, _, ids, _ = R.consolidate(pts, [5, 5, 5], np.zeros((3, 2), np.uint8), K)
    # Fermat point of the right isosceles triangle: all angles 120 degrees; on the diagonal x = y = (3 - sqrt(3)) / 6
    t = (3 - math.sqrt(3)) / 6
    assert abs(gm[0, 0] - t) < 2e-3 and abs(gm[0, 1] - t) < 2e-3 and ids.tolist() == [5]
    # a point coinciding with the start value (the mean): the eps early return gives the mean itself
    pts = np.array([[1.0, 1.0], [0.0, 0.0], [2.0, 2.0], [1.0, 1.0]], np.float32)
    gm, _, _, _ = R.consolidate(pts, [2, 2, 2, 2], np.zeros((4, 1), np.uint8), K)
    assert gm[0].tolist() == [1.0, 1.0]
    # four points of a square: converges to the centre
    pts = np.array([[0, 0], [2, 0], [2, 2], [0, 2.0]], np.float32)
    gm, _, _, _ = R.consolidate(pts, [1, 1, 1, 1], np.zeros((4, 1), np.uint8), K)
    assert np.allclose(gm[0], [1.0, 1.0], atol=1e-6)


# ---- the unpinned choice: exact int64 sums against float accumulation -------------------------------------------------------------

def test_budget_float_accumulation_vs_int64():
    """OpenCV accumulates A and b in float; the restatement sums exactly.  On one KITTI-sized frame (1,000 points per camera pair),
    the tracked points differ by at most 0.05 px where both keep the point (measured 0.016 px: DESIGN.md 2), and status differs on at
    most 0.5 % of the points"""
    fr = synth.tracking_frames(1226, 370, seed=0)
    P = [R.build_pyramid(i) for i in fr["prev"]]
    N = [R.build_pyramid(i) for i in fr["next"]]
    pts = synth.tracking_points(1000, seed=6)
    worst, flips = 0.0, 0
    for cam in range(2):
        a, sa = R.track(P[0], N[cam], pts)
        b, sb = R.track(P[0], N[cam], pts, accumulate="float")
        both = sa & sb
        worst = max(worst, float(np.abs(a[both] - b[both]).max()))
        flips += int((sa != sb).sum())
    print(f"float accumulation vs int64: max |d next_xy| = {worst:.4f} px, status flips = {flips}")
    assert worst <= 0.05, worst
    assert flips <= 0.005 * 2 * len(pts), flips


# ---- the C entry points refuse bad arguments before touching a device ------------------------------------------------------------

def test_entry_points_refuse_bad_arguments_without_a_device():
    build.build_hip()
    lib = api.load_library()
    fake = C.c_void_p(0x1000)                                      # never dereferenced: every check comes first
    buf = (C.c_uint8 * 64)()
    img = (C.c_void_p * 2)(C.c_void_p(0x2000), None)
    assert lib.velo_set_images(None, img, 1, 10, 10, 10) == -1 and b"null ctx" in lib.velo_last_error()
    assert lib.velo_set_images(fake, img, 0, 10, 10, 10) == -1
    assert lib.velo_set_images(fake, img, 9, 10, 10, 10) == -1
    assert lib.velo_set_images(fake, img, 2, 10, 10, 10) == -1 and b"image 1 is null" in lib.velo_last_error()
    assert lib.velo_set_images(fake, img, 1, 10, 10, 9) == -1 and b"stride" in lib.velo_last_error()
    assert lib.velo_set_images(fake, img, 1, 0, 10, 10) == -1
    p = api.lk_params()
    job = (api.VeloTrackJob * 1)(api.VeloTrackJob(0, 0, C.c_void_p(0x3000), 4))
    assert lib.velo_track_features(None, job, 1, C.byref(p), buf, buf, buf) == -1
    assert lib.velo_track_features(fake, job, -1, C.byref(p), buf, buf, buf) == -1
    assert lib.velo_track_features(fake, job, 1, None, buf, buf, buf) == -1
    for bad in (dict(window=20), dict(window=3), dict(window=33), dict(max_level=8), dict(max_count=101), dict(epsilon=-1.0),
                dict(min_eig_threshold=float("nan"))):
        q = api.lk_params(**bad)
        assert lib.velo_track_features(fake, job, 1, C.byref(q), buf, buf, buf) == -1, bad
    assert lib.velo_track_features(fake, None, 0, C.byref(p), None, None, None) == 0          # nothing to do
    neg = (api.VeloTrackJob * 1)(api.VeloTrackJob(0, 0, C.c_void_p(0x3000), -1))
    assert lib.velo_track_features(fake, neg, 1, C.byref(p), buf, buf, buf) == -1 and b"negative" in lib.velo_last_error()
    nul = (api.VeloTrackJob * 1)(api.VeloTrackJob(0, 0, None, 3))
    assert lib.velo_track_features(fake, nul, 1, C.byref(p), buf, buf, buf) == -1 and b"null points" in lib.velo_last_error()
    assert lib.velo_track_features(fake, job, 1, C.byref(p), None, buf, buf) == -1
    dims = (C.c_int32 * 4)()
    assert lib.velo_get_image_level(None, 0, 0, 0, 0, None, 0, dims) == -1
    assert lib.velo_get_image_level(fake, 0, 0, 0, 3, None, 0, dims) == -1


def test_param_struct_layouts_match_the_header(tmp_path):
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = tmp_path / "probe.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "velo_hip.h"\nint main(void) {\n'
                   '  printf("%zu %zu %zu %zu %zu\\n", sizeof(velo_track_job), offsetof(velo_track_job, prev_xy), offsetof(velo_track_job, n),'
                   ' sizeof(velo_lk_params), offsetof(velo_lk_params, flow_outlier));\n  return 0; }\n')
    exe = str(tmp_path / "probe")
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(root, "include"), str(src), "-o", exe], check=True)
    out = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert out == [C.sizeof(api.VeloTrackJob), api.VeloTrackJob.prev_xy.offset, api.VeloTrackJob.n.offset, C.sizeof(api.VeloLkParams),
                   api.VeloLkParams.flow_outlier.offset]
