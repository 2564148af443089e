"""frameToFrame's visual matches assembled on the GPU from resident keypoint frames (velo_frames_*, velo_build_matches[_batch],
velo_get_visual) against tests/visual_ref.py, the restatement of matchUsingId, velo.h:627-654 and the landmark rule.  Everything is
compared for equality: integers, and float bits that are copied or come from the arithmetic velo_landmarks_at_frame already pins."""
import numpy as np
import pytest

import helpers as H
import landmarks_ref as LR
import visual_ref as VR
import velo_amd  # noqa: F401
from velo_amd import api, synth

pytestmark = pytest.mark.gpu
K = VR.CHUNK


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def put(ctx, frame, per_cam):
    for cam, (ids, kps, has, cloud) in enumerate(per_cam):
        ctx.frames_put(frame, cam, ids, kps, has, cloud)


def check(ctx, f1, f2, frame1, frame2, ct, lm=None, pose2_inv=None):
    """build_matches(f1, f2) on ctx equals the restatement on (frame1, frame2): counts, pairs, records"""
    want, want_n = VR.assemble(frame1, frame2, ct, lm)
    per_cam, pairs = ctx.build_matches(f1, f2, pose2_inv)
    got = ctx.get_visual()
    assert per_cam.tolist() == want_n.tolist()
    assert pairs.tolist() == np.stack([want["point1"], want["point2"]], axis=1).tolist()
    assert got.tobytes() == want.tobytes()
    return want


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("sizes", [((0,), (0,)), ((1,), (1,)), ((5,), (0,)), ((0,), (5,)), ((K - 1,), (K - 1,)), ((K,), (K,)),
                                   ((K + 1,), (K + 1,)), ((700,), (3 * K + 1,)), ((3 * K + 1, 0), (40, 300)), ((300, 500), (0, 2 * K))])
def test_sizes_per_camera(ctx, sizes):
    f1, f2, ct = VR.random_pair(100 + sum(sizes[0]) + 7 * sum(sizes[1]), sizes[0], sizes[1])
    ctx.frames_reset(ct)
    put(ctx, 1, f1)
    put(ctx, 0, f2)
    want = check(ctx, 1, 0, f1, f2, ct)
    if min(sizes[0][-1], sizes[1][-1]) >= 5:
        assert len(want) >= 3


def test_id_cases_and_landmark_switch(ctx):
    f1, f2, ct = VR.id_cases()
    ctx.frames_reset(ct)
    put(ctx, 4, f1)
    put(ctx, 3, f2)
    want = check(ctx, 4, 3, f1, f2, ct)                                  # a context without a landmark store
    assert len(want) == 9
    check(ctx, 4, 3, f1, f2, ct, pose2_inv=np.eye(4))                   # ... also when a pose is handed in
    # a landmark store whose id space ends below ids 70000, 80000 and 90000; ids 5, 9 and 11 are added
    ctx.landmarks_reset(ct)
    poses = np.zeros((3, 6))
    poses[:, 5] = [0.0, 0.4, 0.8]
    for f in range(3):
        ctx.landmarks_set_pose(f, poses[f])
        ctx.landmarks_observe(f, 0, [5, 9, 11, 13], np.float32([[.01, .02], [.03, -.01], [-.02, .01], [0, 0]]) + np.float32(.001 * f),
                              [0, 1, -1, -1], np.float32([[.2, .4, 20 - .4 * f], [.9, -.3, 30 - .4 * f]]))
    ids, pts, _ = ctx.landmarks_triangulate(2)
    assert ids.tolist() == [5, 9, 11, 13] and ctx.landmarks_info()["n_ids"] == 14
    check(ctx, 4, 3, f1, f2, ct)                                         # pose2_inv16 == NULL with a store: no substitution
    Minv = np.linalg.inv(api.pose_vec_to_mat(poses[2]))
    Minv[3] = [1e-3, -2e-3, 5e-4, 1.25]
    book = LR.LandmarkBook(1)
    book.observe_frame(2, [np.zeros((4, 2))], [[5, 9, 11, 13]], [[-1] * 4], [np.zeros((0, 3))])
    book.store(ids, pts)
    lm = VR.landmarks_dict(book, Minv, 2)
    want = check(ctx, 4, 3, f1, f2, ct, lm, Minv)
    assert want["d2"].tolist() == [1, 1, 0, 1, 1, 1, 1, 0, 1]            # id 5 at ind2 7 has depth through its landmark only
    ai, ax = ctx.landmarks_at_frame(2, Minv)
    for r in want:
        id = int(f2[0][0][r["point2"]])
        if id in (5, 9, 11):
            assert np.array_equal(bits(r["p3_2"]), bits(ax[ai.tolist().index(id)]))
    fresh = api.Context(0)
    with pytest.raises(api.VeloError, match="velo_frames_reset has not run"):
        fresh.build_matches(1, 0)
    fresh.close()


def test_stale_state(ctx):
    """two calls in a row with different frame1, then the same call twice: the slot table is back at -1 every time"""
    rng = np.random.default_rng(5)
    ct = np.float32([[0, 0, 0], [-.5, 0, 0]])
    pool = np.arange(900)
    fr = {f: [VR.random_camera(rng, n, pool) for n in sizes] for f, sizes in {0: (400, 300), 1: (350, 10), 2: (500, 450)}.items()}
    ctx.frames_reset(ct)
    for f in (2, 0, 1):                                                  # out of order
        put(ctx, f, fr[f])
    a = check(ctx, 1, 0, fr[1], fr[0], ct)
    b = check(ctx, 2, 0, fr[2], fr[0], ct)
    c = check(ctx, 2, 0, fr[2], fr[0], ct)
    assert len(a) > 50 and len(b) > 100 and b.tobytes() == c.tobytes()
    check(ctx, 1, 2, fr[1], fr[2], ct)
    check(ctx, 0, 0, fr[0], fr[0], ct)                                   # a frame against itself: every keypoint matches


def test_frame_store(ctx):
    rng = np.random.default_rng(6)
    ct = np.float32([[0, 0, 0], [-.5, 0, 0]])
    pool = np.arange(3000)
    mk = lambda *sizes: [VR.random_camera(rng, n, pool) for n in sizes]   # noqa: E731
    ctx.frames_reset(ct, arena_capacity=4096)                            # 1,024 words: the arena reallocates on the way
    frames = {3: mk(200, 100), 1: mk(150, 0), 2: mk(300, 250)}
    for f in (3, 1, 2):
        put(ctx, f, frames[f])
    info = ctx.frames_info()
    assert ctx.frames_count(2)[0].tolist() == [300, 250] and ctx.frames_count(2)[1] == 550
    assert ctx.frames_count(1)[0].tolist() == [150, 0] and ctx.frames_count(9)[0].tolist() == [-1, -1] and ctx.frames_count(9)[1] == 0
    assert info["arena_reallocations"] >= 2 and info["frames"] == 3 and info["entries"] == 6 and info["n_cams"] == 2
    check(ctx, 2, 1, frames[2], frames[1], ct)
    check(ctx, 3, 2, frames[3], frames[2], ct)
    # replaced by a smaller entry (in place) and by a larger one (moved): the other frames are untouched
    used = ctx.frames_info()["arena_used"]
    frames[2] = mk(120, 40)
    put(ctx, 2, frames[2])
    assert ctx.frames_info()["arena_used"] == used and ctx.frames_info()["entries"] == 6
    check(ctx, 3, 2, frames[3], frames[2], ct)
    frames[2] = mk(700, 650)
    put(ctx, 2, frames[2])
    assert ctx.frames_info()["arena_used"] > used and ctx.frames_info()["free_blocks"] >= 2
    check(ctx, 3, 2, frames[3], frames[2], ct)
    check(ctx, 2, 1, frames[2], frames[1], ct)
    # a dropped frame is gone until it is put again; its blocks are reused
    ctx.frames_drop(3)
    assert ctx.frames_info()["frames"] == 2
    before = ctx.get_visual().tobytes()
    with pytest.raises(api.VeloError, match="frame 3, camera 0 has not been put"):
        ctx.build_matches(3, 2)
    with pytest.raises(api.VeloError, match="frame 3, camera 0 has not been put"):
        ctx.build_matches(2, 3)
    assert ctx.get_visual().tobytes() == before                          # nothing changed
    ctx.frames_put(3, 0, *frames[3][0])
    with pytest.raises(api.VeloError, match="frame 3, camera 1 has not been put"):
        ctx.build_matches(3, 2)
    used = ctx.frames_info()["arena_used"]
    ctx.frames_put(3, 1, *frames[3][1])
    assert ctx.frames_info()["arena_used"] == used
    check(ctx, 3, 2, frames[3], frames[2], ct)
    with pytest.raises(api.VeloError, match="the store has 2"):
        ctx.frames_put(3, 2, *frames[3][1])


def test_capacity_below_the_count(ctx):
    f1, f2, ct = VR.random_pair(77, (300, 200), (280, 220))
    ctx.frames_reset(ct)
    put(ctx, 1, f1)
    put(ctx, 0, f2)
    want, want_n = VR.assemble(f1, f2, ct)
    per_cam, pairs, n = ctx.build_matches(1, 0, capacity=7)
    assert n == len(want) > 7 and per_cam.tolist() == want_n.tolist() and pairs.shape == (7, 2)
    assert pairs.tolist() == np.stack([want["point1"], want["point2"]], axis=1)[:7].tolist()
    assert ctx.get_visual().tobytes() == want.tobytes()                  # the visual set is complete
    assert ctx.get_visual(capacity=3).tobytes() == want[:3].tobytes()


@pytest.fixture(scope="module")
def landmark_walk():
    """VR.landmark_case() walked on one context: frames 0..5 observed and triangulated on the device, the book fed with the device's points"""
    seq, fr1, fr2 = VR.landmark_case()
    c = api.Context(0)
    c.landmarks_reset(seq["cam_trans"])
    for f in range(len(seq["poses"])):
        c.landmarks_set_pose(f, seq["poses"][f])

    def solve(f, ids):
        for cam, (i, k, h, cl) in enumerate(seq["frames"][f]):
            c.landmarks_observe(f, cam, i, k, h, cl)
        gi, gp, _ = c.landmarks_triangulate(f)
        assert gi.tolist() == list(ids)
        return gp
    book = VR.walk_book(seq, fr2, solve)
    yield dict(seq=seq, ctx=c, book=book, fr1=fr1, fr2=fr2)
    c.close()


def test_landmarks_after_a_sequence_walk(landmark_walk):
    w = landmark_walk
    seq, c, fr1, fr2 = w["seq"], w["ctx"], w["fr1"], w["fr2"]
    Minv = np.linalg.inv(api.pose_vec_to_mat(seq["poses"][fr2]))
    Minv[3] = [1e-3, -2e-3, 5e-4, 1.25]                                  # a general last row: the division by p[3] is exercised
    lm = VR.landmarks_dict(w["book"], Minv, fr2)
    c.frames_reset(seq["cam_trans"])
    put(c, fr2, seq["frames"][fr2])
    put(c, fr1, seq["frames"][fr1])
    want = check(c, fr1, fr2, seq["frames"][fr1], seq["frames"][fr2], seq["cam_trans"], lm, Minv)
    # the occurrence counts the CPU test asserts on made-up points hold with the device's landmarks too
    for combos, replaced, fresh in VR.occurrence_counts(seq["frames"][fr1], seq["frames"][fr2], lm):
        assert all(v >= 5 for v in combos.values()) and replaced >= 5 and fresh >= 5
    # p3_2 of a substituted record has the bits velo_landmarks_at_frame gives for that id
    ai, ax = c.landmarks_at_frame(fr2, Minv)
    at = {int(i): p for i, p in zip(ai, ax)}
    n_sub = 0
    for r in want:
        id = int(seq["frames"][fr2][r["cam"]][0][r["point2"]])
        if id in at:
            assert np.array_equal(bits(r["p3_2"]), bits(at[id]))
            n_sub += 1
    assert 40 < n_sub < len(want) - 40                                   # added and not-added ids are mixed
    check(c, fr1, fr2, seq["frames"][fr1], seq["frames"][fr2], seq["cam_trans"])      # no pose: no substitution


def test_batch_equals_single_calls(landmark_walk):
    """3 contexts: 2 cameras with a landmark store, 1 camera without one, 1 camera with nothing to match; batch and single calls
    alternate over three frame pairs; twins driven by single calls only give the expected bytes."""
    w = landmark_walk
    seq = w["seq"]
    rng = np.random.default_rng(8)
    one = {f: [VR.random_camera(rng, n, np.arange(1500))] for f, n in {4: 600, 5: 2 * K, 6: 333, 7: 50}.items()}
    none = {f: [VR.random_camera(rng, 40, np.arange(100 * f, 100 * f + 80))] for f in (4, 5, 6, 7)}       # disjoint ids
    ct1 = np.float32([[.1, .2, .3]])
    a_batch = w["ctx"]
    a_twin = api.Context(0)
    a_twin.landmarks_reset(seq["cam_trans"])
    for f in range(len(seq["poses"])):
        a_twin.landmarks_set_pose(f, seq["poses"][f])
    for f in range(w["fr2"] + 1):
        for cam, (i, k, h, cl) in enumerate(seq["frames"][f]):
            a_twin.landmarks_observe(f, cam, i, k, h, cl)
        a_twin.landmarks_triangulate(f)
    others = [api.Context(0) for _ in range(4)]
    batch, twins = [a_batch, others[0], others[1]], [a_twin, others[2], others[3]]
    for group in (batch, twins):
        group[0].frames_reset(seq["cam_trans"])
        group[1].frames_reset(ct1, arena_capacity=2048)
        group[2].frames_reset(ct1)
        for f in (4, 5, 6, 7):
            put(group[0], f, seq["frames"][f])
            put(group[1], f, one[f])
            put(group[2], f, none[f])
    poses = [np.linalg.inv(api.pose_vec_to_mat(seq["poses"][f])) for f in range(8)]
    n_batch = [0, 0, 0]
    for step, f1 in enumerate((5, 6, 7)):
        f2 = f1 - 1
        M = [poses[f2]] * 3
        want = []
        for c in twins:
            per_cam, pairs = c.build_matches(f1, f2, poses[f2])
            want.append((per_cam, pairs, c.get_visual()))
        if step % 2 == 0:
            got = api.build_matches_batch(batch, [f1] * 3, [f2] * 3, M)
        else:
            got = [c.build_matches(f1, f2, poses[f2]) for c in batch]
        for k in range(3):
            assert got[k][0].tolist() == want[k][0].tolist() and got[k][1].tolist() == want[k][1].tolist(), (step, k)
            assert batch[k].get_visual().tobytes() == want[k][2].tobytes(), (step, k)
            n_batch[k] += len(want[k][1]) if step % 2 == 0 else 0
        # ... and records AND the pairs the calls wrote (pairs_out of every context) are the restatement's
        def pairs_of(recs):
            return np.stack([recs["point1"], recs["point2"]], axis=1).tolist()
        r1 = VR.assemble(one[f1], one[f2], ct1)[0]
        assert want[1][2].tobytes() == r1.tobytes() and got[1][1].tolist() == pairs_of(r1) and len(r1) > 3, step
        assert got[2][1].tolist() == [] and got[2][0].tolist() == [0], step
        if f2 <= w["fr2"]:                                              # frames the book has walked
            lm = VR.landmarks_dict(w["book"], poses[f2], f2)
            r0, n0 = VR.assemble(seq["frames"][f1], seq["frames"][f2], seq["cam_trans"], lm)
            assert want[0][2].tobytes() == r0.tobytes() and got[0][1].tolist() == pairs_of(r0) and got[0][0].tolist() == n0.tolist(), step
    assert n_batch[0] > 100 and n_batch[1] > 50 and n_batch[2] == 0
    # the raw call: context-major, `capacity` apart, counts per context; the first `capacity` pairs of EVERY context are written
    full = api.build_matches_batch(batch, [6, 6, 6], [5, 5, 5], None)
    per_cam, pairs, n = api.build_matches_batch(batch, [6, 6, 6], [5, 5, 5], None, capacity=4)
    assert per_cam.shape == (3, 8) and pairs.shape == (3, 4, 2) and n[0] > 4 and n[1] > 4 and n[2] == 0
    assert per_cam[0, :2].sum() == n[0] and per_cam[1, 0] == n[1] and not per_cam[:, 2:].any()
    r0 = VR.assemble(seq["frames"][6], seq["frames"][5], seq["cam_trans"])[0]
    r1 = VR.assemble(one[6], one[5], ct1)[0]
    for k, r in ((0, r0), (1, r1)):
        want_pairs = np.stack([r["point1"], r["point2"]], axis=1)
        assert n[k] == len(r) and pairs[k].tolist() == want_pairs[:4].tolist() and full[k][1].tolist() == want_pairs.tolist(), k
        assert batch[k].get_visual().tobytes() == r.tobytes(), k
    assert not pairs[2].any() and full[2][1].tolist() == []
    for c in [a_twin] + others:
        c.close()


def frames_from_records(rec, seed):
    """two frames (2 cameras) whose id join gives the records of synth.stereo_matches back, in shuffled keypoint order and with
    keypoints on either side that match nothing"""
    rng = np.random.default_rng(seed)
    m = api.matches_from_dict(rec)
    f1, f2 = [], []
    for cam in range(2):
        r = m[m["cam"] == cam]
        n = len(r)
        sides = []
        for kp, p3, d, extra_lo in ((r["p2_1"], r["p3_1"], r["d1"], 10000), (r["p2_2"], r["p3_2"], r["d2"], 20000)):
            extra = 17
            ids = np.r_[np.arange(n), extra_lo + np.arange(extra)].astype(np.int32)
            kps = np.vstack([kp, rng.normal(size=(extra, 2)).astype(np.float32) * np.float32(.2)]).astype(np.float32)
            with_depth = np.flatnonzero(np.r_[d != 0, np.zeros(extra, bool)])
            has = np.full(n + extra, -1, dtype=np.int32)
            slot = rng.permutation(len(with_depth))
            has[with_depth] = slot
            cloud = np.zeros((len(with_depth), 3), dtype=np.float32)
            cloud[slot] = p3[with_depth]
            perm = rng.permutation(n + extra)
            sides.append((ids[perm], kps[perm], has[perm], cloud))
        f1.append(sides[0])
        f2.append(sides[1])
    return f1, f2


def test_registration_equals_set_visual():
    """the small pair of the parity tests: velo_frame_to_frame after velo_build_matches and after velo_set_visual(restatement records)
    give bit-equal x, T and summary and equal good matches; the same through velo_frame_to_frame_batch; a LiDAR-only registration of a
    context that never built matches is unchanged"""
    d = H.small_pair(16, 128)
    rec = synth.stereo_matches(n_per_cam=150, mix="all")
    f1, f2 = frames_from_records(rec, 3)
    ct = synth.CAM_TRANS[:2].astype(np.float32)
    want, _ = VR.assemble(f1, f2, ct)
    assert len(want) == 300 and {(int(a), int(b)) for a, b in zip(want["d1"], want["d2"])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    ctxs = [api.Context(0, icp_skip=2) for _ in range(5)]
    for c in ctxs:
        c.set_target(d["tgt_xyz"], d["tgt_off"])
        c.set_source(d["src_xyz"], d["src_off"])

    def result(x, T, s):
        return np.asarray(x).tobytes() + np.asarray(T).tobytes(), bytes(s)
    a, b, lidar = ctxs[0], ctxs[1], ctxs[4]
    lidar_before = result(*lidar.frame_to_frame(d["x0"]))[0]
    a.frames_reset(ct)
    put(a, 1, f1)
    put(a, 0, f2)
    a.build_matches(1, 0)
    b.set_visual(want)
    ra, rb = a.frame_to_frame(d["x0"]), b.frame_to_frame(d["x0"])
    assert result(*ra) == result(*rb) and ra[2].n_solves > 0
    ga, gb = a.good_matches(), b.good_matches()
    assert ga.tobytes() == gb.tobytes() and len(ga) > 0
    # ... and through the batch entry with two contexts
    c2, d2 = ctxs[2], ctxs[3]
    c2.frames_reset(ct)
    put(c2, 1, f1)
    put(c2, 0, f2)
    built = api.build_matches_batch([a, c2], [1, 1], [0, 0])         # the batch build fills both contexts' host-side pairs
    assert all(p.tolist() == np.stack([want["point1"], want["point2"]], axis=1).tolist() for _, p in built)
    b.set_visual(want)
    d2.set_visual(want)
    xa, Ta, Sa = api.frame_to_frame_batch([a, c2], [d["x0"], d["x0"]])
    xb, Tb, Sb = api.frame_to_frame_batch([b, d2], [d["x0"], d["x0"]])
    assert xa.tobytes() == xb.tobytes() and Ta.tobytes() == Tb.tobytes() and [bytes(s) for s in Sa] == [bytes(s) for s in Sb]
    assert a.good_matches().tobytes() == b.good_matches().tobytes() and c2.good_matches().tobytes() == d2.good_matches().tobytes()
    assert len(c2.good_matches()) > 0
    assert result(*lidar.frame_to_frame(d["x0"]))[0] == lidar_before
    for c in ctxs:
        c.close()
