"""velo_frames_put_frame[_batch] -- a frame put with its keypoint depth computed on the GPU -- against TODAY'S ENTRIES on a second
context: velo_project_lidar, velo_depth_association, velo_frames_put, velo_frames_put_descriptors and velo_landmarks_observe, camera
by camera (tests/test_gpu_next_rows.py holds the first two bit-equal to the oracle).  The new call is never its own yardstick.  It
moves integers, copies float bits and runs the SAME device functions as the yardstick, so everything is compared for byte equality:
velo_frames_get, every number of velo_frames_info / velo_frames_desc_info, and the landmark store.  tests/test_frame_depth_cpu.py
shows on the oracle that the cases hold keypoints with and without depth.  Sizes straddle a chunk of the write (256) and a lane chunk
of the ring carry (64)."""
import os

import numpy as np
import pytest

import velo_amd  # noqa: F401
from velo_amd import api, synth
from test_depth_oracle import crafted_rings

pytestmark = pytest.mark.gpu
CT2 = np.ascontiguousarray(synth.CAM_TRANS[:2], np.float32)
W = synth.cam_window()
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "depth_mini.npz")


@pytest.fixture(scope="module")
def pair():
    """(the context under test, the yardstick's context)"""
    a, b = api.Context(0), api.Context(0)
    yield a, b
    a.close()
    b.close()


def make_cam(n, seed, rows=True, window=W, id0=0, nan=False):
    rng = np.random.default_rng(1000 + seed)
    kps = synth.keypoints_in_window(n, seed=seed, window=window)
    if nan and n > 6:
        kps[5] = (np.nan, 0.0)
        kps[6] = (0.0, np.nan)
    ids = id0 + rng.permutation(4 * n + 4)[:n]                           # distinct, not sorted
    return api.FrameCam(ids, kps, window, rng.integers(0, 256, (n, 64), dtype=np.uint8) if rows else None)


def old_way(c, frame, cams, thresh, of_target=False, observe=False, cam_trans=CT2):
    """what the new call replaces, camera by camera; returns n_with_depth per camera"""
    n_wd = []
    for cam, K in enumerate(cams):
        c.project_lidar(of_target, cam_trans[cam], K.window)
        kd, has = c.depth_association(K.keypoints_xy, thresh)
        c.frames_put(frame, cam, K.ids, K.keypoints_xy, has, kd)
        if K.rows is not None:
            c.frames_put_descriptors(frame, cam, K.rows)
        if observe:
            c.landmarks_observe(frame, cam, K.ids, K.keypoints_xy, has, kd)
        n_wd.append(len(kd))
    return n_wd


def entry_bytes(got):
    ids, xy, has, cloud, rows = got
    return (ids.tobytes(), xy.tobytes(), has.tobytes(), cloud.tobytes(), None if rows is None else rows.tobytes(), len(ids), len(cloud))


def frame_state(c, frames):
    """everything the frame store says: every entry of `frames`, both info arrays"""
    out = []
    for f in frames:
        per_cam, _ = c.frames_count(f)
        out.append([entry_bytes(c.frames_get(f, k)) if per_cam[k] >= 0 else None for k in range(len(per_cam))])
    return out, c.frames_info(), c.frames_desc_info()


def lm_state(c, ids):
    xyz, added, cnt = c.landmarks_get(ids)
    return xyz.tobytes(), added.tobytes(), cnt.tobytes(), c.landmarks_info()


def both(pair, frame, cams, thresh=0.2, of_target=False, observe=False, cam_trans=CT2):
    """the call on one context, today's entries on the other: the counts agree; returns them"""
    a, b = pair
    got = a.frames_put_frame(frame, cams, thresh, of_target=of_target, observe=observe)
    want = old_way(b, frame, cams, thresh, of_target, observe, cam_trans)
    assert got.tolist() == want
    return want


def fresh(pair, xyz, off, cam_trans=CT2, arena=0, target=None):
    for c in pair:
        c.set_source(xyz, off)
        if target is not None:
            c.set_target(*target)
        c.frames_reset(cam_trans, arena_capacity=arena)


def test_depth_mini_fixture_one_camera_store_both_sides(pair):
    g = np.load(GOLDEN)
    ct = np.float32(g["cam_t"]).reshape(1, 3)
    xyz, off = crafted_rings(n_rings=20, seed=4)                         # the OTHER side holds another cloud: the side named is the side read
    fresh(pair, xyz, off, ct, target=(g["xyz"], g["off"]))
    ids = np.arange(len(g["keypoints"]), dtype=np.int32)[::-1]
    cams = [api.FrameCam(ids, g["keypoints"], g["window"], None)]
    n_t = both(pair, 0, cams, float(g["thresh"]), of_target=True, cam_trans=ct)
    n_s = both(pair, 1, cams, float(g["thresh"]), of_target=False, cam_trans=ct)
    assert frame_state(pair[0], [0, 1]) == frame_state(pair[1], [0, 1])
    got = pair[0].frames_get(0, 0)
    assert np.array_equal(got[2], g["has_depth"]) and got[3].tobytes() == g["kp_with_depth"].tobytes()      # the oracle's, as recorded
    assert 0 < n_t[0] < len(ids) and len(n_s) == 1
    for c in pair:
        c.set_source(g["xyz"], g["off"])
    both(pair, 1, cams, float(g["thresh"]), of_target=False, cam_trans=ct)
    assert entry_bytes(pair[0].frames_get(1, 0)) == entry_bytes(pair[0].frames_get(0, 0))


@pytest.mark.parametrize("n_rings", [0, 1, 64, 65, 150])
def test_ring_counts_across_the_lane_chunk_carry(pair, n_rings):
    # (no ring: an array of one point that no ring owns -- an empty array has no row stride to hand over)
    xyz, off = crafted_rings(n_rings=n_rings) if n_rings else (np.zeros((1, 3), np.float32), np.zeros(1, np.int32))
    fresh(pair, xyz, off)
    cams = [make_cam(700, 3, nan=True), make_cam(700, 3, id0=5000, nan=True)]
    n_wd = both(pair, 2, cams, 0.2)
    assert frame_state(pair[0], [2]) == frame_state(pair[1], [2])
    if n_rings >= 64:
        assert all(50 <= m <= 650 for m in n_wd)                         # both kinds, in both cameras (test_frame_depth_cpu.py)
    if n_rings <= 1:
        assert n_wd == [0, 0]
    both(pair, 2, cams, synth.DEPTH_ASSOC_THRESH)                        # the reference's threshold, over the same entries
    assert frame_state(pair[0], [2]) == frame_state(pair[1], [2])


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 769])
def test_keypoint_counts_at_the_chunk_edges(pair, n):
    xyz, off = crafted_rings(n_rings=150)
    fresh(pair, xyz, off)
    cams = [make_cam(n, 40 + n, rows=(n != 255)), make_cam(769 - n, 41 + n, id0=9000)]
    n_wd = both(pair, 0, cams, 0.2)
    assert frame_state(pair[0], [0]) == frame_state(pair[1], [0])
    ids, xy, has, cloud, rows = pair[0].frames_get(0, 0)
    assert ids.tobytes() == cams[0].ids.tobytes() and xy.tobytes() == cams[0].keypoints_xy.tobytes()
    assert has[has >= 0].tolist() == list(range(n_wd[0])) and len(cloud) == n_wd[0]     # appended in keypoint order
    assert (rows is None) == (n == 255) and (rows is None or rows.tobytes() == cams[0].rows.tobytes())


def test_empty_window_wide_threshold_and_unequal_cameras(pair):
    xyz, off = crafted_rings(n_rings=150)
    fresh(pair, xyz, off)
    nowhere = np.float64([5.0, 6.0, 5.0, 6.0])                            # nothing projects into it: no depth anywhere
    cams = [api.FrameCam(np.arange(300), synth.keypoints_in_window(300, seed=8), nowhere, None), make_cam(0, 9)]
    assert both(pair, 0, cams, 0.2) == [0, 0]
    wide = [make_cam(520, 10), make_cam(0, 11, rows=False)]              # two cameras of different sizes, one empty
    n_wd = both(pair, 1, wide, 1e9)
    tight = both(pair, 2, wide, 0.2)
    assert n_wd[0] > tight[0] > 0 and n_wd[0] > 520 // 2 and n_wd[1] == 0
    assert frame_state(pair[0], [0, 1, 2]) == frame_state(pair[1], [0, 1, 2])
    assert np.all(pair[0].frames_get(0, 0)[2] == -1) and pair[0].frames_get(1, 1)[4] is None and pair[0].frames_get(0, 1)[4].shape == (0, 64)


def test_small_arena_grows_and_entries_are_replaced(pair):
    xyz, off = crafted_rings(n_rings=150)
    fresh(pair, xyz, off, arena=4096)                                    # 1,024 words, 64 rows: both arenas reallocate on the way
    sizes = {0: (300, 120), 1: (520, 0), 2: (257, 256)}
    for f, (n0, n1) in sizes.items():
        both(pair, f, [make_cam(n0, 60 + f), make_cam(n1, 70 + f, id0=7000)])
    assert pair[0].frames_info()["arena_reallocations"] >= 1 and pair[0].frames_desc_info()["arena_reallocations"] >= 1
    assert frame_state(pair[0], [0, 1, 2]) == frame_state(pair[1], [0, 1, 2])
    # frame 1 replaced by a smaller entry without rows (its old rows go), then by a larger one with rows; the neighbours stay
    both(pair, 1, [make_cam(100, 80, rows=False), make_cam(30, 81, rows=False, id0=7000)])
    assert pair[0].frames_get(1, 0)[4] is None
    assert frame_state(pair[0], [0, 1, 2]) == frame_state(pair[1], [0, 1, 2])
    both(pair, 1, [make_cam(900, 82), make_cam(600, 83, id0=7000)])
    assert frame_state(pair[0], [0, 1, 2]) == frame_state(pair[1], [0, 1, 2])
    # and the old way replaces what the new call put, the new call what the old way put: the stores stay equal
    a, b = pair
    old_way(a, 0, [make_cam(310, 84), make_cam(5, 85, id0=7000)], 0.2)
    b.frames_put_frame(0, [make_cam(310, 84), make_cam(5, 85, id0=7000)], 0.2)
    assert frame_state(a, [0, 1, 2]) == frame_state(b, [0, 1, 2])


def test_observe_feeds_the_landmark_store_and_its_triangulation(pair):
    xyz, off = crafted_rings(n_rings=150)
    fresh(pair, xyz, off)
    for c in pair:
        c.landmarks_reset(CT2, log_capacity=256)                         # the log reallocates on the way
    rng = np.random.default_rng(90)
    all_ids = set()
    for f in range(3):
        for c in pair:
            c.landmarks_set_pose(f, [0.0, 0.002 * f, 0.0, 0.01 * f, 0.0, 0.9 * f])
        cams = []
        for cam in range(2):
            K = make_cam(300, 91 + cam)                                  # the same ids and nearly the same keypoints in every frame
            K.keypoints_xy = np.ascontiguousarray(K.keypoints_xy + np.float32(rng.normal(0, 1e-4, K.keypoints_xy.shape)))
            cams.append(K)
            all_ids |= set(K.ids.tolist())
        both(pair, f, cams, 0.2, observe=True)
    ids = np.array(sorted(all_ids) + [max(all_ids) + 7], np.int32)
    assert lm_state(pair[0], ids) == lm_state(pair[1], ids)
    assert pair[0].landmarks_info()["log_reallocations"] >= 1 and pair[0].landmarks_info()["log_entries"] == 1800
    assert frame_state(pair[0], [0, 1, 2]) == frame_state(pair[1], [0, 1, 2])
    got, want = pair[0].landmarks_triangulate(2), pair[1].landmarks_triangulate(2)
    assert len(got[0]) > 100 and all(g.tobytes() == w.tobytes() for g, w in zip(got, want))
    assert lm_state(pair[0], ids) == lm_state(pair[1], ids)


def test_projection_state_matches_and_registration_are_untouched(pair):
    a, b = pair
    d = synth.scan_pair(16, 128)
    for c in pair:
        c.set_params(icp_skip=1)
    fresh(pair, d["src_xyz"], d["src_off"], target=(d["tgt_xyz"], d["tgt_off"]))
    wide = np.float64([-2.0, 2.0, -1.0, 1.0])
    a.project_lidar(True, CT2[1], wide)
    before = [x.tobytes() for x in a.projection()]
    kps = synth.keypoints_in_window(400, seed=12, window=wide)
    depth_before = [x.tobytes() for x in a.depth_association(kps, 0.3)]
    assert len(depth_before[0]) > 0
    frames = {f: [make_cam(400, 100, window=wide), make_cam(350, 101, window=wide, id0=4000)] for f in (0, 1)}   # the same ids and rows
    for f, cams in frames.items():
        both(pair, f, cams, 0.3, of_target=bool(f))
    assert [x.tobytes() for x in a.projection()] == before
    assert [x.tobytes() for x in a.depth_association(kps, 0.3)] == depth_before
    assert frame_state(a, [0, 1]) == frame_state(b, [0, 1])
    # the matches built against frames put this way are those built against frames put the old way, by id and by descriptor
    for build in (lambda c: c.build_matches(1, 0), lambda c: c.build_matches_desc(1, 0, match_thresh=300.0)):
        (pa, qa), (pb, qb) = build(a), build(b)
        assert pa.tolist() == pb.tolist() and qa.tobytes() == qb.tobytes() and pa.sum() > 100
        assert a.get_visual().tobytes() == b.get_visual().tobytes()
    # a frame1 stamp goes with the entry, as after velo_frames_put
    a.frames_put_frame(1, frames[1], 0.3, of_target=True)
    with pytest.raises(api.VeloError, match="has changed since the visual set was built"):
        a.frames_prune(1)
    # a LiDAR-only registration does not see any of it
    for c in pair:
        c.set_visual(None)
    xa, Ta, _ = a.frame_to_frame(synth.INITIAL_GUESS)
    a.frames_put_frame(0, frames[0], 0.3)
    xa2, Ta2, _ = a.frame_to_frame(synth.INITIAL_GUESS)
    xb, Tb, _ = b.frame_to_frame(synth.INITIAL_GUESS)
    assert xa.tobytes() == xb.tobytes() == xa2.tobytes() and Ta.tobytes() == Tb.tobytes() == Ta2.tobytes()
    for c in pair:
        c.set_params(icp_skip=200)


def test_refusals_change_nothing(pair):
    a, _ = pair
    xyz, off = crafted_rings(n_rings=70)
    a.set_source(xyz, off)
    a.frames_reset(CT2)
    a.landmarks_reset(CT2)
    good = [make_cam(300, 110), make_cam(200, 111, id0=3000)]
    a.frames_put_frame(0, good, 0.2, observe=True)
    ids = np.concatenate([K.ids for K in good])
    state = lambda: (frame_state(a, [0, 1]), lm_state(a, ids))   # noqa: E731
    before = state()

    def cam(ids=None, rows=None, n=300):
        K = make_cam(n, 112, rows=False)
        if ids is not None:
            K.ids = np.ascontiguousarray(ids, np.int32)
        K.rows = rows
        return K
    neg, big, twice = np.arange(300), np.arange(300), np.arange(300)
    neg[7], big[7], twice[7] = -1, 1 << 26, 8
    cases = [([good[0], cam(neg)], False, "negative id"), ([good[0], cam(big)], False, "id 67108864"), ([cam(twice), good[1]], True, "appears twice"),
             (good, True, "observed already")]
    for cams, observe, msg in cases:
        with pytest.raises(api.VeloError, match=msg):
            a.frames_put_frame(1 if msg != "observed already" else 0, cams, 0.2, observe=observe)
    with pytest.raises(api.VeloError, match="frame"):
        a.frames_put_frame(1 << 22, good, 0.2)
    # a null array with n > 0, and more rows than the match key indexes: straight through the C entry
    import ctypes as C
    lib, table = a._lib, (api.VeloFrameCam * 8)()
    table[0], table[1] = good[0].as_struct(), good[1].as_struct()
    table[1].keypoints_xy = None
    assert lib.velo_frames_put_frame(a.handle, 1, 0, C.cast(table, C.c_void_p), 0.2, 0, None) == -1 and b"null ids / keypoints" in lib.velo_last_error()
    n_big = (1 << 22) + 1                                                # one row more than the match key indexes; zero pages nobody reads
    many = api.FrameCam(np.zeros(n_big, np.int32), np.zeros((n_big, 2), np.float32), W, np.zeros((n_big, 64), np.uint8))
    with pytest.raises(api.VeloError, match="descriptor rows"):
        a.frames_put_frame(1, [many, good[1]], 0.2)
    assert state() == before
    # the stores the call needs
    c = api.Context(0)
    with pytest.raises(api.VeloError, match="velo_frames_reset has not run"):
        c.frames_put_frame(0, good, 0.2)
    c.frames_reset(CT2)
    with pytest.raises(api.VeloError, match="no source cloud"):
        c.frames_put_frame(0, good, 0.2)
    c.set_source(xyz, off)
    with pytest.raises(api.VeloError, match="no target cloud"):
        c.frames_put_frame(0, good, 0.2, of_target=True)
    with pytest.raises(api.VeloError, match="velo_landmarks_reset has not run"):
        c.frames_put_frame(0, good, 0.2, observe=True)
    c.landmarks_reset(CT2[:1])
    with pytest.raises(api.VeloError, match="the landmark store has 1 cameras"):
        c.frames_put_frame(0, good, 0.2, observe=True)
    assert c.frames_info()["entries"] == 0 and c.landmarks_info()["log_entries"] == 0
    c.close()


def test_batch_equals_single_on_three_contexts():
    """1 and 2 cameras, different ring counts, a context without keypoints, mixed of_target, batch and single calls alternating"""
    d = synth.scan_pair(16, 128)
    clouds = [crafted_rings(n_rings=150), crafted_rings(n_rings=40, seed=5), (d["src_xyz"], d["src_off"])]
    trans = [CT2, CT2[:1], CT2]
    side = [False, False, True]
    batch, single = [api.Context(0) for _ in range(3)], [api.Context(0) for _ in range(3)]
    for group in (batch, single):
        for i, c in enumerate(group):
            c.set_source(*clouds[i])
            if side[i]:
                c.set_target(d["tgt_xyz"], d["tgt_off"])
            c.frames_reset(trans[i], arena_capacity=4096)
            c.landmarks_reset(trans[i], log_capacity=128)
    wide = np.float64([-2.0, 2.0, -1.0, 1.0])

    def cams_of(f):
        return [[make_cam(700 - 90 * f, 120 + f), make_cam(257, 121 + f, rows=False, id0=6000)],
                [make_cam(0, 122) if f == 0 else make_cam(300, 122 + f)],            # frame 0: a context without keypoints
                [make_cam(256, 123 + f, window=wide), make_cam(130, 124 + f, window=wide, id0=6000)]]
    all_ids = np.arange(0, 9100, dtype=np.int32)
    for f in range(2):
        cams = cams_of(f)
        if f == 0:                                                         # batch first, then singles ...
            got = api.frames_put_frame_batch(batch, [f] * 3, cams, 0.25, side, observe=True)
        else:                                                              # ... then a single call between two batch calls of two
            got = [None] * 3
            got[2] = batch[2].frames_put_frame(f, cams[2], 0.25, of_target=side[2], observe=True)
            got[1], got[0] = api.frames_put_frame_batch([batch[1], batch[0]], [f, f], [cams[1], cams[0]], 0.25, [side[1], side[0]], observe=True)
        want = [single[i].frames_put_frame(f, cams[i], 0.25, of_target=side[i], observe=True) for i in range(3)]
        assert [g.tolist() for g in got] == [w.tolist() for w in want]
        for i in range(3):
            assert frame_state(batch[i], range(f + 1)) == frame_state(single[i], range(f + 1)), (f, i)
            assert lm_state(batch[i], all_ids) == lm_state(single[i], all_ids), (f, i)
    assert sum(int(g.sum()) for g in got) > 100
    # refused as a whole: the third context's frame is out of range, the first two are not touched
    before = [frame_state(c, [0, 1]) for c in batch]
    with pytest.raises(api.VeloError, match="context 2: frame"):
        api.frames_put_frame_batch(batch, [5, 5, -1], cams_of(1), 0.25, side)
    with pytest.raises(api.VeloError, match="context 1"):
        api.frames_put_frame_batch(batch, [5, 5, 5], [cams_of(1)[0], [api.FrameCam([-4], [[0.0, 0.0]], W)], cams_of(1)[2]], 0.25, side)
    assert [frame_state(c, [0, 1]) for c in batch] == before and all(c.frames_count(5)[1] == 0 for c in batch)
    for c in batch + single:
        c.close()
