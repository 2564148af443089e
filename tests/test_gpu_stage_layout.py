"""Every launch set of the visual side whose staged tables are laid out by csrc/velo_stage_layout.h, at the counts where a sum of
offsets can go wrong: empty and one-element tables, counts that straddle a 64-byte line (63 / 64 / 65) and a chunk of the frame
kernels (kFrChunk - 1 / kFrChunk / kFrChunk + 1), an empty camera between full ones, outputs that start unaligned.  Everything is
compared for equality with the Python restatements of tests/ (visual_ref, loop_ref, descriptor_ref, lk_ref, gftt_ref, landmarks_ref,
prune_ref) or, for the put of a frame with its depth, with today's entries camera by camera on a second context
(test_gpu_frame_depth.py).  Small inputs: the whole file takes a few seconds."""
import numpy as np
import pytest

import descriptor_ref as DR
import gftt_ref as G
import landmarks_ref as LR
import lk_ref as LK
import loop_ref as LP
import prune_ref as PR
import visual_ref as VR
import velo_amd  # noqa: F401
from velo_amd import api, synth
from test_depth_oracle import crafted_rings
from test_gpu_frame_depth import CT2, frame_state, lm_state, make_cam, old_way
from test_gpu_frame_prune import entry_bytes, frames_from_records, want_bytes

pytestmark = pytest.mark.gpu
K = VR.CHUNK
IMG_W, IMG_H = 161, 97                      # odd sizes, a few tiles of every image kernel


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def trio(hip_lib):
    """three contexts: [0] leads every batch call and serves the single-context ones"""
    cs = [api.Context(0, icp_skip=2) for _ in range(3)]
    yield cs
    for c in cs:
        c.close()


def put(ctx, frame, per_cam, desc=None):
    for cam, (ids, kps, has, cloud) in enumerate(per_cam):
        ctx.frames_put(frame, cam, ids, kps, has, cloud)
        if desc is not None:
            ctx.frames_put_descriptors(frame, cam, desc[cam])


# (frame1 sizes, frame2 sizes) per context: unequal counts from 0, 1, 63, 64, 65, K - 1, K, K + 1; one camera of every context's pair
# is empty on one side at least once
SIZES_3X2 = [(((1, 64), (63, K)), ((K - 1, 0), (0, 1)), ((K + 1, 65), (65, 64))),
             (((0, K), (K + 1, 0)), ((64, 63), (K - 1, K + 1)), ((65, 1), (1, 0)))]


# ---- velo_build_matches[_batch] ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 65])
def test_build_matches_one_context_one_camera(trio, n):
    c = trio[0]
    f1, f2, ct = VR.random_pair(300 + n, (n,), (n,))
    c.frames_reset(ct)
    put(c, 1, f1)
    put(c, 0, f2)
    want, want_n = VR.assemble(f1, f2, ct)
    per_cam, pairs = c.build_matches(1, 0)
    assert per_cam.tolist() == want_n.tolist()
    assert pairs.tolist() == np.stack([want["point1"], want["point2"]], axis=1).tolist()
    assert c.get_visual().tobytes() == want.tobytes()


@pytest.mark.parametrize("sizes", SIZES_3X2)
def test_build_matches_three_contexts_two_cameras(trio, sizes):
    want = []
    for i, (c, (s1, s2)) in enumerate(zip(trio, sizes)):
        f1, f2, ct = VR.random_pair(310 + 10 * i + sum(s1), s1, s2)
        c.frames_reset(ct)
        put(c, 1, f1)
        put(c, 0, f2)
        want.append(VR.assemble(f1, f2, ct))
    got = api.build_matches_batch(trio, [1] * 3, [0] * 3)
    total = 0
    for c, (per_cam, pairs), (w, w_n) in zip(trio, got, want):
        assert per_cam.tolist() == w_n.tolist()
        assert pairs.tolist() == np.stack([w["point1"], w["point2"]], axis=1).tolist()
        assert c.get_visual().tobytes() == w.tobytes()
        total += len(w)
    assert total > 0


# ---- velo_build_matches_desc[_batch], velo_match_frames -----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 65])
def test_build_matches_desc_one_context_one_camera(trio, n):
    c = trio[0]
    f1, f2, d1, d2, ct = LP.random_pair(320 + n, (n,), (max(n, 1),))
    c.frames_reset(ct)
    put(c, 1, f1, d1)
    put(c, 0, f2, d2)
    want, want_n, _ = LP.assemble(f1, f2, d1, d2, ct)
    per_cam, pairs = c.build_matches_desc(1, 0)
    assert per_cam.tolist() == want_n.tolist() and pairs.tolist() == LP.pairs_of(want).tolist()
    assert c.get_visual().tobytes() == want.tobytes()


@pytest.mark.parametrize("sizes", SIZES_3X2)
def test_build_matches_desc_three_contexts_two_cameras(trio, sizes):
    want, rows = [], []
    for i, (c, (s1, s2)) in enumerate(zip(trio, sizes)):
        f1, f2, d1, d2, ct = LP.random_pair(330 + 10 * i + sum(s1), s1, s2)
        c.frames_reset(ct)
        put(c, 1, f1, d1)
        put(c, 0, f2, d2)
        want.append(LP.assemble(f1, f2, d1, d2, ct))
        rows.append((d1, d2))
    got = api.build_matches_desc_batch(trio, [1] * 3, [0] * 3)
    for c, (per_cam, pairs), (w, w_n, _) in zip(trio, got, want):
        assert per_cam.tolist() == w_n.tolist() and pairs.tolist() == LP.pairs_of(w).tolist()
        assert c.get_visual().tobytes() == w.tobytes()
    # the screening call on the same rows: frame 1 against candidates 0, 1, 0 -- three jobs per camera, no units and no contexts staged
    for c, (d1, d2) in zip(trio, rows):
        n_kept, min_d = c.match_frames(1, [0, 1, 0])
        for k, d in enumerate((d2, d1, d2)):
            for cam in range(2):
                _, _, md, pairs = DR.match(d1[cam], d[cam])
                assert (n_kept[k, cam], min_d[k, cam]) == (len(pairs), md), (k, cam)


# ---- velo_match_descriptors ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shapes", [[(1, 1)], [(7, 5)], [(1, 3), (65, 63), (129, 7)]])
def test_match_descriptors_odd_query_counts(trio, shapes):
    rng = np.random.default_rng(340 + len(shapes) + shapes[0][0])
    jobs = [(LP.rand_rows(rng, nq), LP.rand_rows(rng, nt)) for nq, nt in shapes]
    idx, dist, md, pairs = trio[0].match_descriptor_jobs(jobs)
    for j, (q, t) in enumerate(jobs):
        widx, wdist, wmd, wpairs = DR.match(q, t)
        assert np.array_equal(idx[j], widx) and np.array_equal(dist[j], wdist) and int(md[j]) == wmd and np.array_equal(pairs[j], wpairs), j


# ---- velo_set_images, velo_track_features, velo_detect_features, velo_get_corner_response ------------------------------------------------
@pytest.fixture(scope="module")
def images(trio):
    fr = synth.tracking_frames(IMG_W, IMG_H, seed=7)
    c = trio[0]
    c.set_images(fr["prev"])
    c.set_images(fr["next"])
    return dict(fr=fr, prev=[LK.build_pyramid(i) for i in fr["prev"]], next=[LK.build_pyramid(i) for i in fr["next"]],
                eig=[G.response(i) for i in fr["next"]])


def test_image_levels_of_a_small_odd_frame(trio, images):
    c = trio[0]
    for previous, pyrs in ((True, images["prev"]), (False, images["next"])):
        for cam in range(2):
            for lev, L in enumerate(pyrs[cam]):
                for kind in ("img", "dx", "dy"):
                    assert np.array_equal(c.get_image_level(cam, lev, kind, previous=previous)[0], L[kind]), (previous, cam, lev, kind)


@pytest.mark.parametrize("counts", [(1,), (7,), (1, 7, 0, 7)])
def test_track_jobs_whose_status_and_kept_start_unaligned(trio, images, counts):
    pts = synth.tracking_points(16, IMG_W, IMG_H, seed=11, margin=6.0)
    jobs = [(j % 2, (j // 2) % 2, pts[j:j + n]) for j, n in enumerate(counts)]
    got = trio[0].track_features(jobs)
    for j, (pc, cc, xy) in enumerate(jobs):
        want = LK.track_job(images["prev"][pc], images["next"][cc], xy, win=21, max_level=4)
        assert np.array_equal(bits(got[0][j]), bits(want[0])), j
        assert np.array_equal(got[1][j], want[1]) and np.array_equal(got[2][j], want[2]), j


@pytest.mark.parametrize("n_jobs", [1, 3])
def test_detect_capacity_5(trio, images, n_jobs):
    ex = synth.tracking_points(9, IMG_W, IMG_H, seed=12)
    jobs = [(0, ex), (1, None), (0, ex[:1])][:n_jobs]
    cap = 5
    xy = np.full((n_jobs, cap, 2), -7.0, np.float32)
    resp = np.full((n_jobs, cap), -7.0, np.float32)
    fresh = np.full((n_jobs, cap), 9, np.uint8)
    _, _, _, counts = trio[0].detect_features_raw(jobs, cap, xy, resp, fresh)
    for j, (cam, e) in enumerate(jobs):
        wxy, wv, wfr, wcn = G.detect(images["fr"]["next"][cam], e, eig=images["eig"][cam])
        assert counts[j].tolist() == wcn.tolist() and counts[j, 0] > cap, j
        assert np.array_equal(xy[j], wxy[:cap]) and np.array_equal(bits(resp[j]), bits(wv[:cap])), j
        assert np.array_equal(fresh[j].astype(bool), np.asarray(wfr[:cap], bool)), j


def test_corner_response_of_one_unit(trio, images):
    for cam in range(2):
        assert np.array_equal(bits(trio[0].corner_response(cam)), bits(images["eig"][cam])), cam


# ---- velo_landmarks_observe / _triangulate / _get / _at_frame ----------------------------------------------------------------------------
def test_landmarks_get_and_at_frame_1_and_5_ids(trio):
    c = trio[0]
    ct = np.float32([[0, 0, 0]])
    c.landmarks_reset(ct)
    book = LR.LandmarkBook(1)
    ids5 = [5, 9, 11, 13, 20]
    poses = np.zeros((4, 6))
    poses[:, 5] = [0.0, 0.4, 0.8, 1.2]
    kps = np.float32([[.01, .02], [.03, -.01], [-.02, .01], [0, 0], [.02, .02]])
    cloud = np.float32([[.2, .4, 20], [.9, -.3, 30]])
    for f in range(4):
        c.landmarks_set_pose(f, poses[f])
        ids = ids5 if f < 3 else [9]                                     # frame 3 sees one id only
        k = (kps + np.float32(.001 * f))[:len(ids)]
        has = [0, 1, -1, -1, -1][:len(ids)] if f < 3 else [-1]
        cl = cloud - np.float32([0, 0, .4 * f])
        c.landmarks_observe(f, 0, ids, k, has, cl)
        book.observe_frame(f, [k], [ids], [has], [cl])
    gi, pts, _ = c.landmarks_triangulate(2)
    assert gi.tolist() == ids5 == book.ids_to_triangulate(2)
    book.store(gi, pts)
    for ask in ([9], ids5, [20, 4, 21, 5, 9]):                           # ids never observed and beyond the store read as zeros
        xyz, added, cnt = c.landmarks_get(ask)
        for k, i in enumerate(ask):
            known = i < len(book.landmarks)
            assert np.array_equal(bits(xyz[k]), bits(book.landmarks[i] if known else np.zeros(3))), (ask, i)
            assert bool(added[k]) == (known and book.keypoint_added[i]) and cnt[k] == (book.keypoint_obs_count[i] if known else 0), (ask, i)
    Minv = np.linalg.inv(api.pose_vec_to_mat(poses[2]))
    Minv[3] = [1e-3, -2e-3, 5e-4, 1.25]
    for f, n in ((3, 1), (2, 5)):
        wi, wx = book.landmarks_at_frame(Minv, f)
        got_i, got_x = c.landmarks_at_frame(f, Minv)
        assert len(wi) == n and got_i.tolist() == wi.tolist() and np.array_equal(bits(got_x), bits(wx)), f


# ---- velo_frames_put_frame[_batch] ------------------------------------------------------------------------------------------------------
def test_put_frame_observe_rows_on_one_camera_only():
    """three contexts x two cameras with unequal counts, one camera with rows and one without, one camera empty, observe=True --
    against today's entries camera by camera on three other contexts"""
    xyz, off = crafted_rings(n_rings=70)
    new, old = [api.Context(0) for _ in range(3)], [api.Context(0) for _ in range(3)]
    try:
        for c in new + old:
            c.set_source(xyz, off)
            c.frames_reset(CT2)
            c.landmarks_reset(CT2, log_capacity=64)
            c.landmarks_set_pose(0, np.zeros(6))
        sizes = [(1, 64), (K + 1, 0), (65, K - 1)]
        cams = [[make_cam(n0, 350 + i, rows=True), make_cam(n1, 360 + i, rows=False, id0=9000)] for i, (n0, n1) in enumerate(sizes)]
        got = api.frames_put_frame_batch(new, [0] * 3, cams, 0.2, observe=True)
        for i in range(3):
            want = old_way(old[i], 0, cams[i], 0.2, observe=True)
            assert np.asarray(got[i]).tolist() == want, i
            assert frame_state(new[i], [0]) == frame_state(old[i], [0]), i
            ids = np.sort(np.concatenate([K_.ids for K_ in cams[i]])).astype(np.int32)
            assert lm_state(new[i], ids) == lm_state(old[i], ids), i
            assert new[i].frames_get(0, 0)[4] is not None and new[i].frames_get(0, 1)[4] is None
        assert sum(int(np.sum(g)) for g in got) > 20                    # keypoints with depth among them
        # one context, one camera with rows and one without, on its own
        one = [make_cam(63, 370, rows=False), make_cam(K, 371, rows=True, id0=9000)]
        n_wd = new[0].frames_put_frame(1, one, 0.2, observe=True)
        assert n_wd.tolist() == old_way(old[0], 1, one, 0.2, observe=True)
        assert frame_state(new[0], [0, 1]) == frame_state(old[0], [0, 1])
    finally:
        for c in new + old:
            c.close()


# ---- velo_frames_prune_batch, velo_frames_keep -------------------------------------------------------------------------------------------
def resized(rng, cam, rows, n):
    """the camera cut to its first n keypoints, or filled up to n with keypoints that match nothing"""
    ids, kps, has, cloud = cam
    if n <= len(ids):
        return (ids[:n], kps[:n], has[:n], cloud), rows[:n]
    m = n - len(ids)
    return ((np.r_[ids, 50000 + np.arange(m)].astype(np.int32), np.vstack([kps, rng.normal(size=(m, 2)) * .2]).astype(np.float32),
             np.r_[has, np.full(m, -1)].astype(np.int32), cloud), np.vstack([rows, LP.rand_rows(rng, m)]))


def test_prune_three_contexts_two_cameras_after_a_registration(trio):
    d = synth.scan_pair(16, 128)
    sides = frames_from_records(synth.stereo_matches(60, mix="all"), 4)
    rng = np.random.default_rng(380)
    rows1, rows0 = LP.near_rows(rng, sides[1], sides[0])
    ct = synth.CAM_TRANS[:2].astype(np.float32)
    sizes = [(63, K), (K + 1, 0), (65, K - 1)]                           # frame 1, the pruned one; frame 0 stays as it is
    f1 = []
    for c, ns in zip(trio, sizes):
        c.set_target(d["tgt_xyz"], d["tgt_off"])
        c.set_source(d["src_xyz"], d["src_off"])
        c.frames_reset(ct)
        cams, rows = zip(*[resized(rng, sides[1][cam], rows1[cam], n) for cam, n in enumerate(ns)])
        put(c, 1, cams, rows)
        put(c, 0, sides[0], rows0)
        f1.append((cams, rows))
    for c, (per_cam, _) in zip(trio, api.build_matches_batch(trio, [1] * 3, [0] * 3)):
        assert per_cam.sum() >= 60
        c.frame_to_frame(d["x0"])
    gms = [c.good_matches() for c in trio]
    got = api.frames_prune_batch(trio, [1] * 3)
    for i, (c, (kept, n_wd), gm, (cams, rows)) in enumerate(zip(trio, got, gms, f1)):
        for cam in range(2):
            first = gm["point1"][gm["cam"] == cam]
            want = PR.prune_literal(cams[cam], rows[cam], first)
            assert kept[cam].tolist() == want[2].tolist() and n_wd[cam] == len(want[0][3]), (i, cam)
            assert entry_bytes(c.frames_get(1, cam)) == want_bytes(want[0], want[1]), (i, cam)
            assert entry_bytes(c.frames_get(0, cam)) == want_bytes(sides[0][cam], rows0[cam]), (i, cam)
        assert sum(len(k) for k in kept) > 10, i
    for c in trio:
        c.set_visual(None)


@pytest.mark.parametrize("n,keep", [(1, [0]), (65, [64, 0, 64]), (K + 1, [K, 1, 0]), (5, [])])
def test_keep_lists_behind_the_tables(trio, n, keep):
    c = trio[0]
    rng = np.random.default_rng(390 + n)
    cam, rows = PR.make_camera(rng, n, "mixed")
    c.frames_reset(CT2[:1])
    put(c, 1, [cam], [rows])
    want = PR.prune_literal(cam, rows, keep)
    kept, n_wd = c.frames_keep(1, 0, keep)
    assert kept.tobytes() == want[2].tobytes() and n_wd == len(want[0][3])
    assert entry_bytes(c.frames_get(1, 0)) == want_bytes(want[0], want[1])
