"""The resident landmark store (velo_landmarks_*) against the reference's bookkeeping: a seeded sequence is walked frame by frame
through path A -- tests/landmarks_ref.py (main.cpp:614-679 in Python containers) feeding the stateless velo_triangulate_points --
and path B, the store.  The solve arithmetic and the block order are the same, so everything is compared for equality."""
import numpy as np
import pytest

import helpers as H
import landmarks_ref as LR
import velo_amd  # noqa: F401
from velo_amd import api

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def observe(ctx, f, per_cam):
    for cam, (ids, kps, has, cloud) in enumerate(per_cam):
        ctx.landmarks_observe(f, cam, ids, kps, has, cloud)


def book_observe(book, f, per_cam):
    book.observe_frame(f, [c[1] for c in per_cam], [c[0] for c in per_cam], [c[2] for c in per_cam], [c[3] for c in per_cam])


def path_a_frame(ctx, book, seq, f):
    ids = book.ids_to_triangulate(f)
    if not ids:
        return ids, np.zeros((0, 3), np.float32), np.zeros(0, api.TRI_RESULT_DTYPE)
    obs, off, p0, init = book.csr(ids)
    pts, res = ctx.triangulate_points(seq["poses"], seq["cam_trans"], obs, off, p0, init)
    book.store(ids, pts)
    return ids, pts, res


@pytest.fixture(scope="module")
def walk():
    """Both paths over LR.main_sequence() on one context; what every frame gave, and the context with the finished store."""
    seq = LR.main_sequence()
    ctx = api.Context(0)
    book = LR.LandmarkBook(2)
    ctx.landmarks_reset(seq["cam_trans"], log_capacity=16)          # the log reallocates many times on the way
    F = len(seq["poses"])
    ctx.landmarks_set_pose(7, seq["poses"][40] + 0.3)               # a wrong pose, overwritten before use
    for f in reversed(range(F)):                                    # out of order
        ctx.landmarks_set_pose(f, seq["poses"][f])
    all_ids = np.array(sorted({50, 51, 52, 53, 5, 70000, 70001, 99999} | set(range(100, 300))), dtype=np.int32)
    rows = []
    for f in range(F):
        book_observe(book, f, seq["frames"][f])
        observe(ctx, f, seq["frames"][f])
        want = path_a_frame(ctx, book, seq, f)
        trunc = None
        if f == 58:                                                 # a capacity below the count: everything is solved, 5 are written
            i5, p5, r5, n5 = ctx.landmarks_triangulate(f, capacity=5)
            trunc = (i5, p5, r5, n5)
            got = None
        else:
            got = ctx.landmarks_triangulate(f)
        state = ctx.landmarks_get(all_ids)
        ref_state = (np.array([book.landmarks[i] if i < len(book.landmarks) else np.zeros(3, np.float32) for i in all_ids], dtype=np.float32),
                     np.array([book.keypoint_added[i] if i < len(book.keypoint_added) else False for i in all_ids]),
                     np.array([book.keypoint_obs_count[i] if i < len(book.keypoint_obs_count) else 0 for i in all_ids], dtype=np.int32))
        rows.append(dict(frame=f, want=want, got=got, trunc=trunc, state=state, ref_state=ref_state))
    yield dict(seq=seq, ctx=ctx, book=book, rows=rows, all_ids=all_ids)
    ctx.close()


def test_every_frame_equals_the_reference_bookkeeping(walk):
    n_tri, n_retri, sizes, before = 0, 0, set(), set()
    for r in walk["rows"]:
        ids, pts, res = r["want"]
        if r["got"] is not None:
            gi, gp, gr = r["got"]
            assert gi.tolist() == list(ids), r["frame"]
            assert np.array_equal(bits(gp), bits(pts)), r["frame"]
            assert gr.tobytes() == np.ascontiguousarray(res).tobytes(), r["frame"]
        xyz, added, cnt = r["state"]
        wx, wa, wc = r["ref_state"]
        assert np.array_equal(cnt, wc), r["frame"]
        assert np.array_equal(added, wa), r["frame"]
        assert np.array_equal(bits(xyz), bits(wx)), r["frame"]
        n_tri += len(ids)
        n_retri += len(before & set(ids))
        before |= set(ids)
        sizes |= {int(c) for c in wc}
    assert n_tri > 500 and n_retri > 300                           # landmarks solved again from their stored point
    assert {0, 1, 2, 3, 64, 65, 130} <= sizes
    assert walk["rows"][60]["want"][0] == [] and len(walk["rows"][60]["got"][0]) == 0      # the frame nobody observed
    info = walk["ctx"].landmarks_info()
    assert info["log_reallocations"] >= 3 and info["n_ids"] == 70001 and info["observed"] == 2 * 66
    assert info["log_entries"] == int(walk["rows"][-1]["ref_state"][2].sum())


def test_capacity_below_the_count_reports_the_count(walk):
    r = walk["rows"][58]
    ids, pts, res = r["want"]
    i5, p5, r5, n5 = r["trunc"]
    assert n5 == len(ids) > 5 and len(i5) == 5
    assert i5.tolist() == list(ids[:5]) and np.array_equal(bits(p5), bits(pts[:5])) and r5.tobytes() == np.ascontiguousarray(res[:5]).tobytes()
    # ... and the landmarks beyond the fifth were solved and stored all the same: test_every_frame compares the whole state of frame 58


def test_landmarks_at_frame_equals_the_restatement(walk):
    ctx, book, seq = walk["ctx"], walk["book"], walk["seq"]
    for f in (62, 60, 3):
        Minv = np.linalg.inv(api.pose_vec_to_mat(seq["poses"][f]))
        Minv[3] = [1e-3, -2e-3, 5e-4, 1.25]                        # a general last row: the division by p[3] is exercised
        wi, wx = book.landmarks_at_frame(Minv, f)
        gi, gx = ctx.landmarks_at_frame(f, Minv)
        assert gi.tolist() == wi.tolist() and np.array_equal(bits(gx), bits(wx)), f
        if f == 62:
            assert len(wi) > 50
            ci, cx, n = ctx.landmarks_at_frame(f, Minv, capacity=7)
            assert n == len(wi) and ci.tolist() == wi[:7].tolist() and np.array_equal(bits(cx), bits(wx[:7]))
    assert len(ctx.landmarks_at_frame(60, np.eye(4))[0]) == 0


def test_state_errors(walk):
    ctx = walk["ctx"]
    i, k, h, c = walk["seq"]["frames"][20][0]
    with pytest.raises(api.VeloError, match="observed already"):
        ctx.landmarks_observe(20, 0, i, k, h, c)
    with pytest.raises(api.VeloError, match="the store has 2"):
        ctx.landmarks_observe(70, 2, i, k, h, c)
    fresh = api.Context(0)
    with pytest.raises(api.VeloError, match="velo_landmarks_reset has not run"):
        fresh.landmarks_triangulate(0)
    fresh.landmarks_reset(walk["seq"]["cam_trans"])
    fresh.landmarks_observe(4, 0, [1, 2], np.zeros((2, 2)), [-1, -1])
    with pytest.raises(api.VeloError, match="have no pose"):
        fresh.landmarks_triangulate(4)
    fresh.close()


def test_batch_equals_single_calls():
    """3 contexts with different frame counts, camera counts and LM settings; batch and single calls alternate over 5 frames; the
    third context never has anything to triangulate.  Twins driven by single calls only give the expected bytes."""
    specs = [dict(seed=11, n_frames=5, n_cams=2, ids=range(0, 60), params={}),
             dict(seed=12, n_frames=4, n_cams=1, ids=range(10, 50), params=dict(max_num_iterations=4, loss_thresh_3D2D=0.05, weight_3D2D=3.0)),
             dict(seed=13, n_frames=2, n_cams=1, ids=range(5, 25), params=dict(function_tolerance=1e-3))]
    seqs = [LR.sequence(s["seed"], s["n_frames"], s["n_cams"], list(s["ids"]), first_frame={i: (0, 5) for i in s["ids"]}) for s in specs]
    batch = [api.Context(0, **s["params"]) for s in specs]
    twins = [api.Context(0, **s["params"]) for s in specs]
    for group in (batch, twins):
        for c, q in zip(group, seqs):
            c.landmarks_reset(q["cam_trans"], log_capacity=32)
            for f in range(len(q["poses"])):
                c.landmarks_set_pose(f, q["poses"][f])
    solved, in_batch = [0, 0, 0], [0, 0, 0]
    for f in range(5):
        for group in (batch, twins):
            for c, q in zip(group, seqs):
                if f < len(q["frames"]):
                    observe(c, f, q["frames"][f])
        want = [c.landmarks_triangulate(f) for c in twins]
        got = api.landmarks_triangulate_batch(batch, [f] * 3) if f % 2 == 1 else [c.landmarks_triangulate(f) for c in batch]
        for k in range(3):
            assert got[k][0].tolist() == want[k][0].tolist(), (f, k)
            assert np.array_equal(bits(got[k][1]), bits(want[k][1])) and got[k][2].tobytes() == want[k][2].tobytes(), (f, k)
            solved[k] += len(want[k][0])
            in_batch[k] += len(want[k][0]) if f % 2 == 1 else 0
            ids = np.arange(0, 64, dtype=np.int32)
            a, b = batch[k].landmarks_get(ids), twins[k].landmarks_get(ids)
            assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]), (f, k)
    assert solved[0] > 30 and solved[1] > 15 and solved[2] == 0
    assert in_batch[0] > 30 and in_batch[1] > 15                   # two contexts with different settings shared the batch launches
    # the raw call: context-major, `capacity` apart, counts per context
    ids, pts, res, n = api.landmarks_triangulate_batch(batch, [3, 2, 1], capacity=4)
    assert ids.shape == (3, 4) and n[0] > 4 and n[2] == 0
    for c in batch + twins:
        c.close()


def test_registration_is_untouched_by_the_store(walk):
    d = H.small_pair(16, 128)
    ctx = api.Context(0, icp_skip=2)

    def register():
        ctx.set_target(d["tgt_xyz"], d["tgt_off"])
        ctx.set_source(d["src_xyz"], d["src_off"])
        x, T, _ = ctx.frame_to_frame(d["x0"])
        return np.asarray(x).tobytes() + np.asarray(T).tobytes()
    before = register()
    seq = walk["seq"]
    ctx.landmarks_reset(seq["cam_trans"], log_capacity=64)
    for f in range(54, 58):
        ctx.landmarks_set_pose(f, seq["poses"][f])
        observe(ctx, f, seq["frames"][f])
    assert len(ctx.landmarks_triangulate(57)[0]) > 10
    assert register() == before
    ctx.close()
