"""GPU: the single-context front end (velo_set_images / velo_track_features / velo_detect_features / velo_get_corner_response) runs
on the table-driven kernels of the batch entries: one implementation per stage, the single entries hand it a list of one context.
What that can break, at tiny shapes and against the numpy restatements (tests/lk_ref.py, tests/gftt_ref.py) bit for bit:
camera bases resolved on the host (jobs that name only a high camera, or cameras out of order; prev_cam != cam), the upload staged
behind the unit and level tables (row stride > width, the most cameras a call takes), single and batch calls alternating on one
context, and the diagnostics build's counters, which both call shapes now feed at one header stride."""
import ctypes as C

import numpy as np
import pytest

import gftt_ref as G
import lk_ref as R
import velo_amd  # noqa: F401
from velo_amd import api, synth

pytestmark = pytest.mark.gpu
W, H = 97, 61


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bytes(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_bytes(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def three_cameras(seed):
    """prev / next of a 97 x 61 rig with 3 cameras: the two of synth.tracking_frames and camera 0 seen two pixels further right"""
    fr = synth.tracking_frames(W, H, seed=seed, flat=False)
    return {k: fr[k] + [np.ascontiguousarray(np.roll(fr[k][0], 2, axis=1))] for k in ("prev", "next")}


def slot_levels(c, n_cams, previous):
    """every stored level of one slot {(cam, level, kind): array}, or None when the slot holds no images"""
    try:
        n = c.image_levels(previous=previous)
    except api.VeloError:
        return None
    return {(cam, lev, kind): c.get_image_level(cam, lev, kind, previous=previous)[0]
            for cam in range(n_cams) for lev in range(n) for kind in ("img", "dx", "dy")}


def assert_slot_is(c, imgs, previous, what):
    """the slot against the restatement's pyramids of `imgs` (None: the slot must hold nothing)"""
    got = slot_levels(c, len(imgs) if imgs is not None else 1, previous)
    if imgs is None:
        assert got is None, what
        return
    assert got is not None, what
    for cam, im in enumerate(imgs):
        pyr = R.build_pyramid(im)
        assert c.image_levels(previous=previous) == len(pyr), (what, cam)
        for lev, L in enumerate(pyr):
            for kind in ("img", "dx", "dy"):
                assert np.array_equal(got[(cam, lev, kind)], L[kind]), (what, cam, lev, kind)


def assert_same_state(a, b, n_cams, what):
    for previous in (False, True):
        la, lb = slot_levels(a, n_cams, previous), slot_levels(b, n_cams, previous)
        assert (la is None) == (lb is None), (what, previous)
        if la is not None:
            assert la.keys() == lb.keys() and all(np.array_equal(la[k], lb[k]) for k in la), (what, previous)


def assert_detect_is(got, counts, jobs, imgs, **params):
    """one detect result per job against gftt_ref.detect on that job's camera"""
    for j, (cam, ex) in enumerate(jobs):
        xy, v, fr, cn = G.detect(imgs[cam], ex, params.get("max_corners", 3000), 0.001, params.get("min_distance", 12.0))
        assert counts[j].tolist() == cn.tolist(), j
        assert np.array_equal(got[j][0], xy) and np.array_equal(bits(got[j][1]), bits(v)) and np.array_equal(got[j][2], fr), j


def assert_track_is(got, jobs, prev, nxt):
    P = [R.build_pyramid(im) for im in prev]
    N = [R.build_pyramid(im) for im in nxt]
    for j, (pc, cc, xy) in enumerate(jobs):
        ref = R.track_job(P[pc], N[cc], xy)
        assert np.array_equal(bits(got[0][j]), bits(ref[0])), j
        assert np.array_equal(got[1][j], ref[1]) and np.array_equal(got[2][j], ref[2]), j


@pytest.fixture(scope="module")
def rig(hip_lib):
    fr = three_cameras(900)
    c = api.Context(0)
    c.set_images(fr["prev"])
    c.set_images(fr["next"])
    yield dict(ctx=c, frames=fr)
    c.close()


def test_detect_jobs_that_name_only_a_high_camera_or_cameras_out_of_order(rig):
    ex = synth.tracking_points(40, W, H, seed=31)
    for jobs in ([(2, ex)], [(2, ex), (0, None)]):
        got, counts = rig["ctx"].detect_features(jobs, return_counts=True, min_distance=5.0)
        assert (counts[:, 0] > 0).all()
        assert_detect_is(got, counts, jobs, rig["frames"]["next"], min_distance=5.0)


def test_track_jobs_between_different_cameras(rig):
    pts = synth.tracking_points(66, W, H, seed=32, margin=4.0)
    jobs = [(2, 0, pts[:65]), (1, 2, pts[65:])]
    got = rig["ctx"].track_features(jobs)
    assert [len(g) for g in got[0]] == [65, 1] and got[1][0].any()
    assert_track_is(got, jobs, rig["frames"]["prev"], rig["frames"]["next"])


def set_images_strided(c, imgs, stride):
    """velo_set_images with rows `stride` bytes apart; what lies between the rows is not the image's"""
    h, w = imgs[0].shape
    held = []
    for k, im in enumerate(imgs):
        buf = np.full((h, stride), 255 - 17 * k, np.uint8)
        buf[:, :w] = im
        held.append(buf)
    ptrs = (C.c_void_p * len(held))(*[b.ctypes.data for b in held])
    st = c._lib.velo_set_images(c.handle, C.cast(ptrs, C.c_void_p), len(held), w, h, stride)
    assert st == 0, c._lib.velo_last_error()                  # (the rows are in the call's own staging buffer when it returns)


@pytest.mark.parametrize("shape", ["three_97x61", "eight_33x17"])
def test_strided_upload_every_level_and_the_response_map(hip_lib, shape):
    if shape == "three_97x61":
        imgs, stride, cams = three_cameras(901)["next"], W + 11, (0, 2)
    else:
        imgs = [synth.render_texture(33, 17, seed=910 + k, n_blobs=60) for k in range(8)]      # kLkMaxCams cameras
        stride, cams = 33 + 31, (0, 7)
    c = api.Context(0)
    try:
        set_images_strided(c, imgs, stride)
        assert_slot_is(c, imgs, False, shape)
        assert_slot_is(c, None, True, shape)                   # one frame only: no previous images yet
        for cam in cams:
            assert np.array_equal(bits(c.corner_response(cam)), bits(G.response(imgs[cam]))), (shape, cam)
    finally:
        c.close()


def test_single_and_batch_calls_alternate_on_one_context(hip_lib):
    """single upload, batch upload in a list of 2, single track, batch detect: after every step the context equals one that only ever
    saw single calls, and the restatement"""
    f = three_cameras(902)
    f = {k: v[:2] for k, v in f.items()}
    g = [synth.render_texture(64, 48, seed=920 + k, n_blobs=200) for k in range(2)]      # the other context of the list: another size
    mix, ref, other, other_ref = (api.Context(0) for _ in range(4))
    pts = synth.tracking_points(70, W, H, seed=33, margin=3.0)
    try:
        mix.set_images(f["prev"])                              # 1. single upload
        ref.set_images(f["prev"])
        assert_same_state(mix, ref, 2, "single upload")
        assert_slot_is(mix, f["prev"], False, "single upload")
        assert_slot_is(mix, None, True, "single upload")
        api.set_images_batch([other, mix], [g, f["next"]])     # 2. batch upload; the context is the second of the list
        ref.set_images(f["next"])
        other_ref.set_images(g)
        assert_same_state(mix, ref, 2, "batch upload")
        assert_same_state(other, other_ref, 2, "batch upload, other")
        assert_slot_is(mix, f["next"], False, "batch upload")
        assert_slot_is(mix, f["prev"], True, "batch upload")
        tjobs = [(0, 1, pts[:65]), (1, 1, pts[65:]), (1, 0, pts[:0])]
        got = mix.track_features(tjobs)                        # 3. single track
        assert same_bytes(got, ref.track_features(tjobs))
        assert_track_is(got, tjobs, f["prev"], f["next"])
        assert_same_state(mix, ref, 2, "single track")
        djobs = [(1, 1, pts), (0, 0, None), (1, 0, pts[:1]), (0, 1, None)]
        dgot, dcounts = api.detect_features_batch([other, mix], djobs, return_counts=True, min_distance=5.0)      # 4. batch detect
        mine = [j for j, job in enumerate(djobs) if job[0] == 1]
        theirs = [j for j, job in enumerate(djobs) if job[0] == 0]
        want, wcounts = ref.detect_features([djobs[j][1:] for j in mine], return_counts=True, min_distance=5.0)
        assert same_bytes([dgot[j] for j in mine], want) and np.array_equal(dcounts[mine], wcounts)
        want, wcounts = other_ref.detect_features([djobs[j][1:] for j in theirs], return_counts=True, min_distance=5.0)
        assert same_bytes([dgot[j] for j in theirs], want) and np.array_equal(dcounts[theirs], wcounts)
        assert_detect_is([dgot[j] for j in mine], dcounts[mine], [djobs[j][1:] for j in mine], f["next"], min_distance=5.0)
        assert_detect_is([dgot[j] for j in theirs], dcounts[theirs], [djobs[j][1:] for j in theirs], g, min_distance=5.0)
        assert_same_state(mix, ref, 2, "batch detect")
        assert_same_state(other, other_ref, 2, "batch detect, other")
    finally:
        for c in (mix, ref, other, other_ref):
            c.close()


def test_diagnostics_counters_after_single_and_after_batch_calls(hip_lib, diag_lib):
    detect_counters = diag_lib.velo_diag_detect_counters
    detect_counters.restype, detect_counters.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int]
    track_counters = diag_lib.velo_diag_track_counters
    track_counters.restype, track_counters.argtypes = C.c_int, [C.c_void_p, C.c_void_p, C.c_int]
    f = three_cameras(903)
    g = [synth.render_texture(64, 48, seed=930 + k, n_blobs=200) for k in range(2)]
    a, b = api.Context(0, lib=diag_lib), api.Context(0, lib=diag_lib)

    def units_of(c):
        hdr = np.full((8, 8), -1, dtype=np.int32)              # kGfHdr ints per unit: [1] candidates, [3] corners
        n = detect_counters(c.handle, C.c_void_p(hdr.ctypes.data), 8)
        return n, hdr

    try:
        a.set_images(f["prev"][:2])
        a.set_images(f["next"][:2])
        b.set_images(g)
        ex = synth.tracking_points(30, W, H, seed=34)
        jobs = [(1, ex), (0, None)]                            # units in the order the jobs name them: camera 1, camera 0
        a.detect_features(jobs, min_distance=5.0)
        n, hdr = units_of(a)
        assert n == 2
        for u, (cam, e) in enumerate(jobs):
            cn = G.detect(f["next"][cam], e, 3000, 0.001, 5.0)[3]
            assert cn[0] > 0 and (int(hdr[u, 1]), int(hdr[u, 3])) == (int(cn[2]), int(cn[0])), u
        bjobs = [(1, 0, None), (0, 1, ex), (1, 1, None), (0, 1, None)]          # 3 units: (b, 0), (a, 1), (b, 1); a lends
        api.detect_features_batch([a, b], bjobs, min_distance=5.0)
        n, hdr = units_of(a)
        assert n == 3
        for u, (ci, cam) in enumerate([(1, 0), (0, 1), (1, 1)]):
            cn = G.detect((f["next"], g)[ci][cam], None, 3000, 0.001, 5.0)[3]
            assert cn[0] > 0 and (int(hdr[u, 1]), int(hdr[u, 3])) == (int(cn[2]), int(cn[0])), u
        a.track_features([(0, 1, synth.tracking_points(65, W, H, seed=35, margin=4.0))])
        cnt = np.zeros(16, dtype=np.uint64)                    # [level] iterations, [8 + level] points that entered the loop
        assert track_counters(a.handle, C.c_void_p(cnt.ctypes.data), 1) == 0
        assert cnt[0] > 0 and 0 < cnt[8] <= 65
        assert track_counters(a.handle, C.c_void_p(cnt.ctypes.data), 0) == 0
        assert not cnt.any()
    finally:
        a.close()
        b.close()
