"""GPU: resident images and pyramidal Lucas-Kanade tracking (velo_set_images / velo_track_features, trackFeatures velo.h:28-116) against
the numpy restatement tests/lk_ref.py: every stored pyramid and derivative level, border included, ARRAY-EQUAL; next_xy FLOAT-BIT-EQUAL
and status / kept ARRAY-EQUAL on one frame's 4 jobs x 3,000 points at 1226 x 370, at an odd-width size, at other window sizes and with
job sizes 0 / 1 / 65 / 20,000, non-finite points; set_images rotates current into previous; registrations are unchanged by image and
track calls; the C++ adaptor (include/velo_track_features.hpp) appends and consolidates what the restatement gives."""
import numpy as np
import pytest

import lk_ref as R
import velo_amd  # noqa: F401
from velo_amd import api, synth

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def kitti():
    fr = synth.tracking_frames(1226, 370, seed=0)
    return dict(fr=fr, prev=[R.build_pyramid(i) for i in fr["prev"]], next=[R.build_pyramid(i) for i in fr["next"]])


@pytest.fixture(scope="module")
def ctx(hip_lib, kitti):
    c = api.Context(0)
    c.set_images(kitti["fr"]["prev"])
    c.set_images(kitti["fr"]["next"])
    yield c
    c.close()


def check_jobs(ctx, prev_pyrs, next_pyrs, jobs, **params):
    got = ctx.track_features(jobs, **params)
    for j, (pc, cc, xy) in enumerate(jobs):
        want = R.track_job(prev_pyrs[pc], next_pyrs[cc], xy, win=params.get("window", 21), max_level=params.get("max_level", 4))
        assert np.array_equal(bits(got[0][j]), bits(want[0])), (j, np.nonzero(bits(got[0][j]) != bits(want[0]))[0][:10])
        assert np.array_equal(got[1][j], want[1]), j
        assert np.array_equal(got[2][j], want[2]), j
    return got


def test_every_level_array_equal(ctx, kitti):
    assert ctx.image_levels() == len(kitti["next"][0]) == 7
    for previous, pyrs in ((True, kitti["prev"]), (False, kitti["next"])):
        for cam in range(2):
            for lev, L in enumerate(pyrs[cam]):
                for kind in ("img", "dx", "dy"):
                    got, pad = ctx.get_image_level(cam, lev, kind, previous=previous)
                    assert pad == R.PAD
                    assert np.array_equal(got, L[kind]), (previous, cam, lev, kind)


def test_one_frame_4_jobs_3000_points(ctx, kitti):
    """main.cpp:222-235: for cam, for prev_cam, 3,000 keypoints of prev_cam (corner_count, kitti.h:7)"""
    pts = [synth.tracking_points(3000, seed=5 + c) for c in range(2)]
    jobs = [(pc, cc, pts[pc]) for cc in range(2) for pc in range(2)]
    got = check_jobs(ctx, kitti["prev"], kitti["next"], jobs)
    assert got[2][0].mean() > 0.9 and 0 < got[1][0].sum() < 3000      # most kept; the flat patches and borders lose some


def test_odd_width_and_other_windows(hip_lib):
    fr = synth.tracking_frames(641, 203, seed=3, flat=True)
    P = [R.build_pyramid(i) for i in fr["prev"]]
    N = [R.build_pyramid(i) for i in fr["next"]]
    c = api.Context(0)
    try:
        c.set_images(fr["prev"])
        c.set_images(fr["next"])
        for cam in range(2):
            for lev in range(len(N[cam])):
                assert np.array_equal(c.get_image_level(cam, lev, "dy")[0], N[cam][lev]["dy"])
                assert np.array_equal(c.get_image_level(cam, lev, "img", previous=True)[0], P[cam][lev]["img"])
        pts = synth.tracking_points(700, 641, 203, seed=11, margin=-8.0)      # some start outside the image
        jobs = [(0, 0, pts), (1, 0, pts[:300]), (0, 1, pts[300:])]
        check_jobs(c, P, N, jobs)
        for win, ml in ((5, 4), (9, 3), (15, 2), (31, 5), (23, 0)):
            check_jobs(c, P, N, jobs, window=win, max_level=ml)
    finally:
        c.close()


def test_kitti_sizes_build(hip_lib):
    for w, h in ((1241, 376), (1242, 375)):
        img = synth.render_texture(w, h, seed=1, n_blobs=300)
        c = api.Context(0)
        try:
            c.set_images([img])
            for lev, L in enumerate(R.build_pyramid(img)):
                for kind in ("img", "dx", "dy"):
                    assert np.array_equal(c.get_image_level(0, lev, kind)[0], L[kind]), (w, h, lev, kind)
        finally:
            c.close()


def test_job_sizes_0_1_65_20000(ctx, kitti):
    big = synth.tracking_points(20000, seed=21, margin=-5.0)
    jobs = [(0, 1, big[:0]), (1, 1, big[:1]), (0, 0, big[1:66]), (1, 0, big), (0, 1, big[:0])]
    got = check_jobs(ctx, kitti["prev"], kitti["next"], jobs)
    assert [len(g) for g in got[0]] == [0, 1, 65, 20000, 0]


def test_set_images_rotates_current_into_previous(hip_lib):
    a = [synth.render_texture(200, 120, seed=s, n_blobs=80) for s in (7, 8)]
    b = [synth.render_texture(200, 120, seed=s, n_blobs=80) for s in (9, 10)]
    c = api.Context(0)
    try:
        c.set_images(a)
        with pytest.raises(api.VeloError):
            c.get_image_level(0, 0, previous=True)                  # one frame only: no previous images yet
        c.set_images(b)
        for cam in range(2):
            assert np.array_equal(c.get_image_level(cam, 0, previous=True)[0], R.pad_reflect(a[cam]))
            assert np.array_equal(c.get_image_level(cam, 0)[0], R.pad_reflect(b[cam]))
        c.set_images(a)
        assert np.array_equal(c.get_image_level(1, 0, previous=True)[0], R.pad_reflect(b[1]))
        with pytest.raises(api.VeloError):
            c.set_images([np.zeros((50, 60), np.uint8)])
            c.track_features([(0, 0, np.zeros((1, 2), np.float32))])   # previous 200 x 120, current 60 x 50
    finally:
        c.close()


def test_tracking_between_registrations_changes_nothing(hip_lib, kitti):
    d = synth.scan_pair(n_beams=16, n_azimuth=128)
    pts = synth.tracking_points(500, seed=4)
    jobs = [(0, 0, pts), (1, 1, pts)]

    def counts(s):
        return (s.n_solves, s.n_assoc_rounds, s.n_queries, s.n_target,
                [(s.solves[i].lm_iterations, s.solves[i].termination) for i in range(s.n_solves)])

    plain = api.Context(0, icp_skip=1)
    mixed = api.Context(0, icp_skip=1)
    try:
        plain.set_target(d["tgt_xyz"], d["tgt_off"])
        plain.set_source(d["src_xyz"], d["src_off"])
        xa, Ta, sa = plain.frame_to_frame(d["x0"])
        mixed.set_images(kitti["fr"]["prev"])
        mixed.set_target(d["tgt_xyz"], d["tgt_off"])
        mixed.set_images(kitti["fr"]["next"])
        mixed.track_features(jobs)
        mixed.set_source(d["src_xyz"], d["src_off"])
        xb, Tb, sb = mixed.frame_to_frame(d["x0"])
        mixed.track_features(jobs)
        xc, Tc, sc = mixed.frame_to_frame(d["x0"])
        xd, Td, sd = plain.frame_to_frame(d["x0"])
    finally:
        plain.close()
        mixed.close()
    assert np.array_equal(xa, xb) and np.array_equal(Ta, Tb) and counts(sa) == counts(sb)
    assert np.array_equal(xc, xd) and np.array_equal(Tc, Td) and counts(sc) == counts(sd)


def test_cxx_adaptor_appends_what_python_and_the_restatement_give(tmp_path, hip_lib):
    """include/velo_track_features.hpp: trackFeaturesFrame (4 jobs, one call) appends to frame 1 what the restatement's tracking and the
    append loop of velo.h:107-114 give; consolidateFeatures then equals the restatement's consolidation; a single trackFeatures call
    with the reference's parameter list does the same for one pair; an image that was not uploaded is refused"""
    import struct
    import subprocess
    from test_track_cpu import K, check_lists, compile_track_driver, parse_lists
    exe = compile_track_driver(tmp_path)
    w, h = 320, 160
    fr = synth.tracking_frames(w, h, seed=4, disparity=4.5)
    P = [R.build_pyramid(i) for i in fr["prev"]]
    N = [R.build_pyramid(i) for i in fr["next"]]
    Ks = [K, (K + np.array([[2, 0, -3], [0, 2, 1.5], [0, 0, 0]], np.float32)).astype(np.float32)]
    Kinv = [np.linalg.inv(k.astype(np.float64)).astype(np.float32) for k in Ks]
    pts = [synth.tracking_points(400, w, h, seed=30 + c, margin=-4.0) for c in range(2)]
    ids = [np.arange(400), np.arange(200, 600)]                       # ids 200..399 seen by both cameras: pairs after tracking
    rng = np.random.default_rng(9)
    desc = [rng.integers(0, 256, (400, 64), dtype=np.uint8) for _ in range(2)]
    case = str(tmp_path / "track.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("iii", 2, w, h))
        for im in fr["prev"] + fr["next"]:
            f.write(np.ascontiguousarray(im).tobytes())
        for c in range(2):
            f.write(Ks[c].tobytes())
            f.write(Kinv[c].tobytes())
        for c in range(2):
            f.write(struct.pack("i", 400))
            f.write(pts[c].astype(np.float32).tobytes())
            f.write(ids[c].astype(np.int32).tobytes())
            f.write(desc[c].tobytes())
    out = subprocess.run([exe, case, "track"], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = parse_lists(out.stdout)

    def appended(jobs):
        kp, kp_p, kid, kd = [], [], [], []
        for pc, cc in jobs:
            nxt, _, kept = R.track_job(P[pc], N[cc], pts[pc])
            for i in np.nonzero(kept)[0]:
                kp_p.append(nxt[i])
                kp.append(R.mat3_apply(Kinv[cc], nxt[i, 0], nxt[i, 1]))
                kid.append(int(ids[pc][i]))
                kd.append(desc[pc][i])
        return kp, kp_p, kid, np.asarray(kd, np.uint8).reshape(-1, 64)

    for cam in range(2):
        kp, kp_p, kid, kd = appended([(0, cam), (1, cam)])              # main.cpp:222-235: prev_cam inner
        assert 0.8 * 800 < len(kid) < 800
        check_lists(got, "frame", cam, (kp, kp_p, kid, kd))
        want = R.consolidate(kp, kid, kd, Ks[cam])
        assert len(want[2]) < len(kid)                                   # ids seen twice were merged
        check_lists(got, "cons", cam, want)
    check_lists(got, "single", 0, appended([(1, 0)]))
    assert got["mismatch_throws"][0].tolist() == [1]


def test_non_finite_points_lose_their_status_like_the_restatement(ctx, kitti):
    """a NaN or infinite coordinate fails the bounds test at every level (cvFloor gives INT_MIN): status 0, not kept; finite points of
    the same call unchanged"""
    pts = synth.tracking_points(64, seed=40)
    pts[[3, 17, 40]] = [[np.nan, 100], [300, np.inf], [-np.inf, np.nan]]
    got = ctx.track_features([(0, 1, pts)])
    want = R.track_job(kitti["prev"][0], kitti["next"][1], pts)
    fin = np.isfinite(pts).all(1)
    assert np.array_equal(bits(got[0][0][fin]), bits(want[0][fin]))
    assert np.array_equal(np.isnan(got[0][0]), np.isnan(want[0]))
    assert np.array_equal(got[1][0], want[1]) and np.array_equal(got[2][0], want[2])
    assert not got[1][0][~fin].any() and not got[2][0][~fin].any()


def test_image_level_read_back_refuses_a_negative_capacity(ctx, hip_lib):
    import ctypes as C
    dims = (C.c_int32 * 4)()
    buf = (C.c_uint8 * 16)()
    assert hip_lib.velo_get_image_level(ctx.handle, 0, 0, 0, 0, buf, -1, dims) == -1
    assert b"negative capacity" in hip_lib.velo_last_error()
    assert hip_lib.velo_get_image_level(ctx.handle, 0, 0, 0, 0, buf, 16, dims) == -1       # too small: refused, nothing written
