"""The visual set of a loop-closure edge built on the GPU from resident descriptor rows (velo_frames_put_descriptors,
velo_build_matches_desc[_batch], velo_match_frames) against tests/loop_ref.py, the restatement of matchFeatures (velo.h:499-560) and
the gather of velo.h:627-654.  Everything is compared for equality: integers, and float bits that are copied or come from the
arithmetic velo_landmarks_at_frame already pins.  The shapes straddle the MFMA query tile (64), a scan chunk of the filter (256) and
the train tile (512)."""
import numpy as np
import pytest

import descriptor_ref as DR
import helpers as H
import loop_ref as LP
import visual_ref as VR
import velo_amd  # noqa: F401
from velo_amd import api, synth
from test_gpu_visual_assembly import frames_from_records

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def put(ctx, frame, per_cam, desc=None):
    for cam, (ids, kps, has, cloud) in enumerate(per_cam):
        ctx.frames_put(frame, cam, ids, kps, has, cloud)
        if desc is not None:
            ctx.frames_put_descriptors(frame, cam, desc[cam])


def check(ctx, f1, f2, frame1, frame2, d1, d2, ct, lm=None, pose2_inv=None, thresh=29.0):
    """build_matches_desc(f1, f2) on ctx equals the restatement on (frame1, frame2): counts, pairs, records"""
    want, want_n, _ = LP.assemble(frame1, frame2, d1, d2, ct, lm, thresh)
    per_cam, pairs = ctx.build_matches_desc(f1, f2, pose2_inv, thresh)
    got = ctx.get_visual()
    assert per_cam.tolist() == want_n.tolist()
    assert pairs.tolist() == LP.pairs_of(want).tolist()
    assert got.tobytes() == want.tobytes()
    return want


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


TILE_SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 769]
SIZES = [((n,), (300,)) for n in TILE_SIZES] + [((300,), (n,)) for n in TILE_SIZES] + [((300, 0), (200, 150)), ((257, 65), (0, 513))]


@pytest.mark.parametrize("sizes", SIZES)
def test_sizes_per_camera(ctx, sizes):
    f1, f2, d1, d2, ct = LP.random_pair(200 + sum(sizes[0]) + 7 * sum(sizes[1]), sizes[0], sizes[1])
    ctx.frames_reset(ct)
    put(ctx, 1, f1, d1)
    put(ctx, 0, f2, d2)
    want = check(ctx, 1, 0, f1, f2, d1, d2, ct)
    if min(sizes[0][0], sizes[1][0]) >= 63:
        assert 10 <= len(want) < sum(sizes[0])                            # the filter keeps and drops


def cams(rng, *sizes):
    return [VR.random_camera(rng, n, np.arange(4000)) for n in sizes]


def test_matching_semantics(ctx):
    rng = np.random.default_rng(11)
    ct = np.float32([[0, 0, 0], [-.5, 0, 0]])
    # duplicated train rows, far apart in index: the lowest index; camera 1: an all-equal train set
    base = LP.rand_rows(rng, 300)
    t0 = np.concatenate([base, base[::-1], base])
    q0 = LP.flip_bits(rng, base[rng.permutation(300)[:200]], rng.integers(0, 5, 200))
    t1 = np.repeat(base[:1], 600, axis=0)
    q1 = LP.flip_bits(rng, np.repeat(base[:1], 70, axis=0), rng.integers(0, 40, 70))
    f1, f2 = cams(rng, 200, 70), cams(rng, 900, 600)
    ctx.frames_reset(ct)
    put(ctx, 1, f1, [q0, q1])
    put(ctx, 0, f2, [t0, t1])
    want = check(ctx, 1, 0, f1, f2, [q0, q1], [t0, t1], ct)
    assert (want["point2"][want["cam"] == 0] < 300).all() and (want["point2"][want["cam"] == 1] == 0).all() and (want["cam"] == 1).sum() > 20
    # all-zero and all-one rows: distances 0 and 512
    z, o = np.zeros((1, 64), np.uint8), np.full((1, 64), 255, np.uint8)
    qa, ta = np.concatenate([z, o, z]), np.concatenate([o, o])
    qb, tb = z.copy(), o.copy()
    f1, f2 = cams(rng, 3, 1), cams(rng, 2, 1)
    put(ctx, 3, f1, [qa, qb])
    put(ctx, 2, f2, [ta, tb])
    for thresh, n in ((29.0, [1, 1]), (512.0, [3, 1]), (511.0, [1, 1])):      # camera 1: min_dist 512, the bound is 768
        want = check(ctx, 3, 2, f1, f2, [qa, qb], [ta, tb], ct, thresh=thresh)
        assert [int((want["cam"] == c).sum()) for c in (0, 1)] == n
    kept, md = ctx.match_frames(3, [2])
    assert md.tolist() == [[0, 512]] and kept.tolist() == [[1, 1]]
    # a camera whose min_dist is 0 and one whose every distance exceeds match_thresh (random rows: the bound is 1.5 min_dist)
    f1, f2, d1, d2, _ = LP.random_pair(12, (400, 300), (350, 280))
    d1[1] = LP.rand_rows(rng, 300)
    put(ctx, 5, f1, d1)
    put(ctx, 4, f2, d2)
    for thresh in (0.0, 29.0, 512.0, float("inf")):
        want = check(ctx, 5, 4, f1, f2, d1, d2, ct, thresh=thresh)
        _, _, md = LP.assemble(f1, f2, d1, d2, ct, None, thresh)
        assert md[0] == 0 and md[1] > 100
        n0, n1 = int((want["cam"] == 0).sum()), int((want["cam"] == 1).sum())
        assert (0 < n0 < 400 if thresh <= 29 else n0 == 400) and n1 == 300      # camera 1: every nearest row lies within 1.5 min_dist
        assert ctx.match_frames(5, [4], thresh)[1].tolist() == [md.tolist()]


@pytest.fixture(scope="module")
def landmark_walk():
    """LP.landmark_case() walked on one context: frames 0..5 observed and triangulated on the device, the book fed with the device's points"""
    seq, fr1, fr2, desc = LP.landmark_case()
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
    yield dict(seq=seq, ctx=c, book=book, fr1=fr1, fr2=fr2, desc=desc)
    c.close()


def test_landmarks_after_a_sequence_walk(landmark_walk):
    w = landmark_walk
    seq, c, fr1, fr2, desc = w["seq"], w["ctx"], w["fr1"], w["fr2"], w["desc"]
    F1, F2 = seq["frames"][fr1], seq["frames"][fr2]
    Minv = np.linalg.inv(api.pose_vec_to_mat(seq["poses"][fr2]))
    Minv[3] = [1e-3, -2e-3, 5e-4, 1.25]                                  # a general last row: the division by p[3] is exercised
    lm = VR.landmarks_dict(w["book"], Minv, fr2)
    c.frames_reset(seq["cam_trans"])
    put(c, fr2, F2, desc[fr2])
    put(c, fr1, F1, desc[fr1])
    want = check(c, fr1, fr2, F1, F2, desc[fr1], desc[fr2], seq["cam_trans"], lm, Minv)
    # the occurrence conditions the CPU test asserts on made-up points hold with the device's landmarks too
    pairs, _ = LP.match_cameras(desc[fr1], desc[fr2])
    for combos, replaced, fresh in LP.occurrence_counts(F1, F2, pairs, lm):
        assert all(v >= 5 for v in combos.values()) and replaced >= 5 and fresh >= 5
    # p3_2 of a substituted record has the bits velo_landmarks_at_frame gives for that id
    ai, ax = c.landmarks_at_frame(fr2, Minv)
    at = {int(i): p for i, p in zip(ai, ax)}
    n_sub = 0
    for r in want:
        id = int(F2[r["cam"]][0][r["point2"]])
        if id in at:
            assert np.array_equal(bits(r["p3_2"]), bits(at[id]))
            n_sub += 1
    assert 40 < n_sub < len(want) - 40                                   # added and not-added ids are mixed
    check(c, fr1, fr2, F1, F2, desc[fr1], desc[fr2], seq["cam_trans"])   # a store and no pose: no substitution


def test_ids_beyond_the_store_and_no_store(ctx):
    f1, f2, ct = VR.id_cases()
    d1, d2 = LP.near_rows(np.random.default_rng(13), f1, f2)
    ctx.frames_reset(ct)
    put(ctx, 4, f1, d1)
    put(ctx, 3, f2, d2)
    want = check(ctx, 4, 3, f1, f2, d1, d2, ct, thresh=45.0)             # a context without a landmark store
    assert len(want) == 10                                               # every query whose id frame2 holds has that row within 40 bits
    check(ctx, 4, 3, f1, f2, d1, d2, ct, pose2_inv=np.eye(4), thresh=45.0)   # ... also when a pose is handed in
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
    check(ctx, 4, 3, f1, f2, d1, d2, ct, thresh=45.0)                    # pose2_inv16 == NULL with a store: no substitution
    Minv = np.linalg.inv(api.pose_vec_to_mat(poses[2]))
    Minv[3] = [1e-3, -2e-3, 5e-4, 1.25]
    import landmarks_ref as LR
    book = LR.LandmarkBook(1)
    book.observe_frame(2, [np.zeros((4, 2))], [[5, 9, 11, 13]], [[-1] * 4], [np.zeros((0, 3))])
    book.store(ids, pts)
    lm = VR.landmarks_dict(book, Minv, 2)
    want = check(ctx, 4, 3, f1, f2, d1, d2, ct, lm, Minv, thresh=45.0)
    sub = [int(f2[0][0][p]) in (5, 9, 11) for p in want["point2"]]
    assert sum(sub) >= 4 and all(want["d2"][k] == 1 for k in range(len(want)) if sub[k])
    assert {70000, 80000, 90000} <= {int(f2[0][0][p]) for p in want["point2"]}
    fresh = api.Context(0)
    with pytest.raises(api.VeloError, match="velo_frames_reset has not run"):
        fresh.build_matches_desc(1, 0)
    fresh.close()


def test_state(ctx):
    rng = np.random.default_rng(14)
    ct = np.float32([[0, 0, 0], [-.5, 0, 0]])
    ctx.frames_reset(ct, arena_capacity=4096)                            # 64 rows: the row arena reallocates on the way
    assert ctx.frames_desc_info() == dict(entries=0, arena_bytes=4096, arena_reallocations=0, free_blocks=0)
    fr, ds = {}, {}
    fr[1], fr[0], ds[1], ds[0], _ = LP.random_pair(15, (200, 100), (150, 90))
    fr[3], fr[2], ds[3], ds[2], _ = LP.random_pair(16, (300, 0), (260, 70))
    for f in (3, 0, 2, 1):                                               # out of order
        put(ctx, f, fr[f])
    before = ctx.frames_info()
    with pytest.raises(api.VeloError, match="frame 1, camera 0 has no descriptor rows"):
        ctx.build_matches_desc(1, 0)
    for f in (3, 0, 2, 1):
        for cam in (1, 0):
            ctx.frames_put_descriptors(f, cam, ds[f][cam])
    info = ctx.frames_desc_info()
    assert info["entries"] == 8 and info["arena_reallocations"] >= 2 and info["arena_bytes"] >= 64 * 1170
    assert ctx.frames_info() == before                                   # the keypoint arena does not know of the rows
    a = check(ctx, 1, 0, fr[1], fr[0], ds[1], ds[0], ct)
    b = check(ctx, 3, 2, fr[3], fr[2], ds[3], ds[2], ct)
    c = check(ctx, 3, 2, fr[3], fr[2], ds[3], ds[2], ct)                 # the same call twice: the same bytes
    assert len(a) > 40 and len(b) > 40 and b.tobytes() == c.tobytes()
    check(ctx, 2, 3, fr[2], fr[3], ds[2], ds[3], ct)                     # the sides swapped
    check(ctx, 0, 0, fr[0], fr[0], ds[0], ds[0], ct)                     # a frame against itself: every keypoint, distance 0
    # refusals leave everything as it is
    shown = ctx.get_visual().tobytes()
    with pytest.raises(api.VeloError, match="91 descriptor rows for the 90 keypoints"):
        ctx.frames_put_descriptors(0, 1, LP.rand_rows(rng, 91))
    with pytest.raises(api.VeloError, match="frame 7, camera 0 has not been put"):
        ctx.frames_put_descriptors(7, 0, LP.rand_rows(rng, 3))
    assert ctx.frames_desc_info() == info and ctx.get_visual().tobytes() == shown
    # rows replaced by a second put_descriptors (in place: the same size)
    ds[0] = [LP.flip_bits(rng, d, rng.integers(0, 30, len(d))) for d in ds[0]]
    for cam in (0, 1):
        ctx.frames_put_descriptors(0, cam, ds[0][cam])
    assert ctx.frames_desc_info() == info
    check(ctx, 1, 0, fr[1], fr[0], ds[1], ds[0], ct)
    # frames_put drops the rows: the next build is refused and the visual set is unchanged
    shown = ctx.get_visual().tobytes()
    ctx.frames_put(1, 0, *fr[1][0])
    assert ctx.frames_desc_info()["entries"] == 7 and ctx.frames_desc_info()["free_blocks"] == info["free_blocks"] + 1
    for pair in ((1, 0), (0, 1)):
        with pytest.raises(api.VeloError, match="frame 1, camera 0 has no descriptor rows") as e:
            ctx.build_matches_desc(*pair)
        assert "-3" in str(e.value)                                      # VELO_ERR_STATE
    with pytest.raises(api.VeloError, match="frame 1, camera 0 has no descriptor rows"):
        ctx.match_frames(0, [2, 1])
    assert ctx.get_visual().tobytes() == shown
    ctx.frames_put_descriptors(1, 0, ds[1][0])                           # the freed block is taken again
    assert ctx.frames_desc_info() == info
    check(ctx, 1, 0, fr[1], fr[0], ds[1], ds[0], ct)
    # a dropped frame takes its rows along; put again, it works again
    ctx.frames_drop(2)
    assert ctx.frames_desc_info()["entries"] == 6
    with pytest.raises(api.VeloError, match="frame 2, camera 0 has not been put"):
        ctx.build_matches_desc(3, 2)
    put(ctx, 2, fr[2], ds[2])
    assert ctx.frames_desc_info()["arena_bytes"] == info["arena_bytes"]
    check(ctx, 3, 2, fr[3], fr[2], ds[3], ds[2], ct)
    keypoint_side = ctx.frames_info()
    for _ in range(3):
        ctx.frames_put_descriptors(3, 0, ds[3][0])
    assert ctx.frames_info() == keypoint_side
    ctx.frames_reset(ct)                                                 # both arenas are empty
    assert ctx.frames_desc_info() == dict(entries=0, arena_bytes=1 << 20, arena_reallocations=0, free_blocks=0)


def test_agreement_with_match_descriptors_and_build_matches(ctx):
    f1, f2, d1, d2, ct = LP.random_pair(17, (700, 300), (600, 513))
    ctx.frames_reset(ct)
    put(ctx, 1, f1)
    put(ctx, 0, f2)
    by_id_before = (ctx.build_matches(1, 0), ctx.get_visual().tobytes())
    for cam in (0, 1):
        ctx.frames_put_descriptors(1, cam, d1[cam])
        ctx.frames_put_descriptors(0, cam, d2[cam])
    per_cam, pairs = ctx.build_matches_desc(1, 0)
    kept, md = ctx.match_frames(1, [0])
    off = 0
    for cam in (0, 1):
        _, _, m, p = ctx.match_descriptors(d1[cam], d2[cam])
        assert pairs[off:off + per_cam[cam]].tolist() == p.tolist() and md[0, cam] == m and kept[0, cam] == len(p) == per_cam[cam]
        off += per_cam[cam]
    # matchUsingId on the same frames gives what it gave before the rows came
    again = (ctx.build_matches(1, 0), ctx.get_visual().tobytes())
    want, _ = VR.assemble(f1, f2, ct)
    assert again[1] == by_id_before[1] == want.tobytes()
    assert all(np.array_equal(a, b) for a, b in zip(again[0], by_id_before[0]))


def test_registration_equals_set_visual():
    """the small pair of the parity tests: velo_frame_to_frame after velo_build_matches_desc and after velo_set_visual(restatement
    records) give bit-equal x, T and summary and equal good matches; the same through velo_frame_to_frame_batch; a LiDAR-only
    registration of a context that never built matches is unchanged"""
    d = H.small_pair(16, 128)
    rec = synth.stereo_matches(n_per_cam=150, mix="all")
    f1, f2 = frames_from_records(rec, 3)
    ct = synth.CAM_TRANS[:2].astype(np.float32)
    rows = LP.rows_by_id(18, [c[0] for c in f1] + [c[0] for c in f2])    # a distinct row per id: the id join, in query order
    d1, d2 = rows[:2], rows[2:]
    want, _, _ = LP.assemble(f1, f2, d1, d2, ct)
    assert len(want) == 300 and {(int(a), int(b)) for a, b in zip(want["d1"], want["d2"])} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    ctxs = [api.Context(0, icp_skip=2) for _ in range(5)]
    for c in ctxs:
        c.set_target(d["tgt_xyz"], d["tgt_off"])
        c.set_source(d["src_xyz"], d["src_off"])

    def result(x, T, s):
        return np.asarray(x).tobytes() + np.asarray(T).tobytes(), bytes(s)
    a, b, c2, d2c, lidar = ctxs
    lidar_before = result(*lidar.frame_to_frame(d["x0"]))[0]
    for c in (a, c2):
        c.frames_reset(ct)
        put(c, 1, f1, d1)
        put(c, 0, f2, d2)
    a.build_matches_desc(1, 0)
    b.set_visual(want)
    ra, rb = a.frame_to_frame(d["x0"]), b.frame_to_frame(d["x0"])
    assert result(*ra) == result(*rb) and ra[2].n_solves > 0
    ga, gb = a.good_matches(), b.good_matches()
    assert ga.tobytes() == gb.tobytes() and len(ga) > 0
    # ... and through the batch entries with two contexts
    built = api.build_matches_desc_batch([a, c2], [1, 1], [0, 0])
    assert all(p.tolist() == LP.pairs_of(want).tolist() for _, p in built)
    b.set_visual(want)
    d2c.set_visual(want)
    xa, Ta, Sa = api.frame_to_frame_batch([a, c2], [d["x0"], d["x0"]])
    xb, Tb, Sb = api.frame_to_frame_batch([b, d2c], [d["x0"], d["x0"]])
    assert xa.tobytes() == xb.tobytes() and Ta.tobytes() == Tb.tobytes() and [bytes(s) for s in Sa] == [bytes(s) for s in Sb]
    assert a.good_matches().tobytes() == b.good_matches().tobytes() and c2.good_matches().tobytes() == d2c.good_matches().tobytes()
    assert len(c2.good_matches()) > 0
    assert result(*lidar.frame_to_frame(d["x0"]))[0] == lidar_before
    for c in ctxs:
        c.close()


def test_screening(ctx):
    rng = np.random.default_rng(19)
    ct = np.float32([[0, 0, 0], [-.5, 0, 0]])
    f1, f2, d1, d2, _ = LP.random_pair(20, (513, 300), (400, 257))
    ctx.frames_reset(ct)
    put(ctx, 9, f1, d1)
    put(ctx, 8, f2, d2)
    cand = {8: d2, 9: d1}                                                # 9: frame1 itself, every distance 0
    for f, sizes in ((3, (65, 0)), (5, (700, 120)), (6, (1, 769))):      # 3: an empty camera
        cand[f] = [LP.rand_rows(rng, n) for n in sizes]
        cand[f][0][:min(sizes[0], 60)] = LP.flip_bits(rng, d1[0][:min(sizes[0], 60)], rng.integers(0, 41, min(sizes[0], 60)))
        put(ctx, f, cams(rng, *sizes), cand[f])
    ctx.build_matches_desc(9, 8)
    shown = ctx.get_visual().tobytes()
    order = [5, 9, 3, 8, 6]
    kept, md = ctx.match_frames(9, order)
    assert kept.shape == md.shape == (5, 2)
    for k, f in enumerate(order):
        for cam in (0, 1):
            _, _, m, p = ctx.match_descriptors(d1[cam], cand[f][cam])
            assert (md[k, cam], kept[k, cam]) == (m, len(p)), (f, cam)
    assert kept[1].tolist() == [513, 300] and md[1].tolist() == [0, 0] and md[2, 1] == -1 and kept[2, 1] == 0 and kept[:, 0].min() > 0
    assert ctx.get_visual().tobytes() == shown                           # the visual set is left alone
    kept, md = ctx.match_frames(9, [])
    assert kept.shape == md.shape == (0, 2) and ctx.get_visual().tobytes() == shown


def test_batch_equals_single_calls(landmark_walk):
    """3 contexts: 2 cameras with a landmark store, 1 camera without one, 1 camera with nothing to match (an empty train side); batch
    and single calls alternate over three frame pairs; twins driven by single calls only give the expected bytes."""
    w = landmark_walk
    seq = w["seq"]
    rng = np.random.default_rng(21)
    ds = {f: LP.rows_by_id(41, [c[0] for c in seq["frames"][f]]) for f in (4, 5, 6, 7)}
    ds = {f: [LP.flip_bits(rng, r, rng.integers(0, 41, len(r))) for r in rows] for f, rows in ds.items()}
    one = {f: cams(rng, n) for f, n in {4: 600, 5: 513, 6: 333, 7: 50}.items()}
    one_d = {4: [LP.rand_rows(rng, 600)]}
    for f, n in ((5, 513), (6, 333), (7, 50)):
        one_d[f] = [LP.flip_bits(rng, one_d[f - 1][0][rng.permutation(len(one_d[f - 1][0]))[:n]], rng.integers(0, 41, n))]
    none = {f: cams(rng, 0 if f < 7 else 40) for f in (4, 5, 6, 7)}
    none_d = {f: [LP.rand_rows(rng, len(none[f][0][0]))] for f in none}
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
            put(group[0], f, seq["frames"][f], ds[f])
            put(group[1], f, one[f], one_d[f])
            put(group[2], f, none[f], none_d[f])
    poses = [np.linalg.inv(api.pose_vec_to_mat(seq["poses"][f])) for f in range(8)]
    n_batch = [0, 0, 0]
    for step, f1 in enumerate((5, 6, 7)):
        f2 = f1 - 1
        want = []
        for c in twins:
            per_cam, pairs = c.build_matches_desc(f1, f2, poses[f2])
            want.append((per_cam, pairs, c.get_visual()))
        if step % 2 == 0:
            got = api.build_matches_desc_batch(batch, [f1] * 3, [f2] * 3, [poses[f2]] * 3)
        else:
            got = [c.build_matches_desc(f1, f2, poses[f2]) for c in batch]
        for k in range(3):
            assert got[k][0].tolist() == want[k][0].tolist() and got[k][1].tolist() == want[k][1].tolist(), (step, k)
            assert batch[k].get_visual().tobytes() == want[k][2].tobytes(), (step, k)
            n_batch[k] += len(want[k][1]) if step % 2 == 0 else 0
        r1 = LP.assemble(one[f1], one[f2], one_d[f1], one_d[f2], ct1)[0]
        assert want[1][2].tobytes() == r1.tobytes() and got[1][1].tolist() == LP.pairs_of(r1).tolist() and len(r1) > 3, step
        assert got[2][1].tolist() == [] and got[2][0].tolist() == [0], step
        if f2 <= w["fr2"]:                                              # frames the book has walked
            lm = VR.landmarks_dict(w["book"], poses[f2], f2)
            r0, n0, _ = LP.assemble(seq["frames"][f1], seq["frames"][f2], ds[f1], ds[f2], seq["cam_trans"], lm)
            assert want[0][2].tobytes() == r0.tobytes() and got[0][1].tolist() == LP.pairs_of(r0).tolist() and got[0][0].tolist() == n0.tolist(), step
    assert n_batch[0] > 100 and n_batch[1] > 50 and n_batch[2] == 0
    # the raw call: context-major, `capacity` apart, counts per context; the first `capacity` pairs of EVERY context are written
    full = api.build_matches_desc_batch(batch, [6, 6, 6], [5, 5, 5], None)
    per_cam, pairs, n = api.build_matches_desc_batch(batch, [6, 6, 6], [5, 5, 5], None, capacity=4)
    assert per_cam.shape == (3, 8) and pairs.shape == (3, 4, 2) and n[0] > 4 and n[1] > 4 and n[2] == 0
    assert per_cam[0, :2].sum() == n[0] and per_cam[1, 0] == n[1] and not per_cam[:, 2:].any()
    r0 = LP.assemble(seq["frames"][6], seq["frames"][5], ds[6], ds[5], seq["cam_trans"])[0]
    r1 = LP.assemble(one[6], one[5], one_d[6], one_d[5], ct1)[0]
    for k, r in ((0, r0), (1, r1)):
        assert n[k] == len(r) and pairs[k].tolist() == LP.pairs_of(r)[:4].tolist() and full[k][1].tolist() == LP.pairs_of(r).tolist(), k
        assert batch[k].get_visual().tobytes() == r.tobytes(), k
    assert not pairs[2].any() and full[2][1].tolist() == []
    for c in [a_twin] + others:
        c.close()


def test_capacity_below_the_count(ctx):
    f1, f2, d1, d2, ct = LP.random_pair(22, (300, 200), (280, 220))
    ctx.frames_reset(ct)
    put(ctx, 1, f1, d1)
    put(ctx, 0, f2, d2)
    want, want_n, _ = LP.assemble(f1, f2, d1, d2, ct)
    per_cam, pairs, n = ctx.build_matches_desc(1, 0, capacity=7)
    assert n == len(want) > 7 and per_cam.tolist() == want_n.tolist() and pairs.shape == (7, 2)
    assert pairs.tolist() == LP.pairs_of(want)[:7].tolist()
    assert ctx.get_visual().tobytes() == want.tobytes()                  # the visual set is complete
    assert ctx.get_visual(capacity=3).tobytes() == want[:3].tobytes()
