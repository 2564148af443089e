"""Resident keypoint frames pruned on the GPU (velo_frames_get, velo_frames_keep, velo_frames_prune[_batch]) against
tests/prune_ref.py, the transcription of removeSlightlyLessTerribleFeatures (velo.h:272-327).  The prune moves integers and copies
float bits and descriptor bytes, so everything is compared for byte equality.  Sizes straddle a chunk of the compaction (256)."""
import numpy as np
import pytest

import loop_ref as LP
import prune_ref as PR
import visual_ref as VR
import velo_amd  # noqa: F401
from velo_amd import api, synth

pytestmark = pytest.mark.gpu
CT2 = np.float32([[0, 0, 0], [-.5, 0, 0]])


@pytest.fixture(scope="module")
def ctx():
    c = api.Context(0)
    yield c
    c.close()


def put(c, frame, cams, rows=None):
    for cam, (ids, kps, has, cloud) in enumerate(cams):
        c.frames_put(frame, cam, ids, kps, has, cloud)
        if rows is not None and rows[cam] is not None:
            c.frames_put_descriptors(frame, cam, rows[cam])


def entry_bytes(got):
    ids, xy, has, cloud, rows = got
    return (ids.tobytes(), xy.tobytes(), has.tobytes(), cloud.tobytes(), None if rows is None else rows.tobytes(),
            len(ids), len(cloud))


def want_bytes(cam, rows):
    ids, kps, has, cloud = cam
    f32 = lambda a, w: np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, w))   # noqa: E731
    return (np.asarray(ids, np.int32).tobytes(), f32(kps, 2).tobytes(), np.asarray(has, np.int32).tobytes(), f32(cloud, 3).tobytes(),
            None if rows is None else np.asarray(rows, np.uint8).tobytes(), len(ids), len(f32(cloud, 3)))


def snapshot(c, frame):
    """everything the store says about `frame`"""
    per_cam, total = c.frames_count(frame)
    return [entry_bytes(c.frames_get(frame, cam)) if per_cam[cam] >= 0 else None for cam in range(len(per_cam))], per_cam.tolist(), total


def keep_and_check(c, frame, cam_idx, cam, rows, keep):
    """frames_keep on the entry equals prune_ref, the literal and the vectorised one; returns the pruned (camera, rows)"""
    want = PR.prune_literal(cam, rows, keep)
    assert PR.same(want, PR.prune_vectorised(cam, rows, keep))
    kept, n_wd = c.frames_keep(frame, cam_idx, keep)
    assert kept.tobytes() == want[2].tobytes() and n_wd == len(want[0][3])
    assert entry_bytes(c.frames_get(frame, cam_idx)) == want_bytes(want[0], want[1])
    assert c.frames_count(frame)[0][cam_idx] == len(want[2])
    return want[0], want[1]


def test_put_get_round_trip(ctx):
    rng = np.random.default_rng(20)
    ctx.frames_reset(CT2)
    cams, rows = zip(*[PR.make_camera(rng, n, "mixed", with_rows=(n != 300)) for n in (300, 0)])
    put(ctx, 3, cams, rows)
    for cam in range(2):
        assert entry_bytes(ctx.frames_get(3, cam)) == want_bytes(cams[cam], rows[cam])
    assert ctx.frames_get(3, 0)[4] is None and ctx.frames_get(3, 1)[4].shape == (0, 64)
    with pytest.raises(api.VeloError, match="frame 4, camera 0 has not been put"):
        ctx.frames_get(4, 0)
    fresh = api.Context(0)
    with pytest.raises(api.VeloError, match="velo_frames_reset has not run"):
        fresh.frames_get(0, 0)
    fresh.close()


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 769])
def test_sizes_and_keep_sets(ctx, n):
    rng = np.random.default_rng(30 + n)
    cam, rows = PR.make_camera(rng, n, "mixed")
    sets = PR.keep_sets(rng, n)
    if n == 769:
        sets["all_but_first"] = np.arange(1, n, dtype=np.int32)          # every item moves by one across every chunk boundary
    ctx.frames_reset(CT2[:1])
    for name, keep in sets.items():
        put(ctx, 1, [cam], [rows])
        pruned, _ = keep_and_check(ctx, 1, 0, cam, rows, keep)
        if name == "half" and n >= 255:
            assert 0 < len(pruned[0]) < n and len(keep) > len(pruned[0])
    put(ctx, 1, [cam], [rows])
    ctx.frames_keep(1, 0, [])
    ctx.frames_keep(1, 0, [])                                            # an emptied entry still counts as put
    assert ctx.frames_count(1)[0].tolist() == [0] and len(ctx.frames_get(1, 0)[0]) == 0


@pytest.mark.parametrize("mode,n", [("none", 300), ("all", 300), ("shared", 4), ("shared", 40)])
def test_has_depth_cases(ctx, mode, n):
    rng = np.random.default_rng(40 + n)
    cam, rows = PR.make_camera(rng, n, mode)
    ctx.frames_reset(CT2[:1], arena_capacity=4096)
    put(ctx, 0, [cam], [rows])
    put(ctx, 1, [cam], [rows])                                           # a neighbour behind the entry: a longer cloud has to move
    used = ctx.frames_info()["arena_used"]
    keep = np.arange(n) if mode == "shared" else PR.keep_sets(rng, n)["half"]
    pruned, _ = keep_and_check(ctx, 0, 0, cam, rows, keep)
    if mode == "shared":
        assert len(cam[3]) == 1 and len(pruned[3]) == n                  # every keypoint got its copy: the cloud GREW
        assert (ctx.frames_info()["arena_used"] > used) == (n == 40)     # 4 n + 3 n words no longer fit the block of 4 n + 3 at n = 40
    assert entry_bytes(ctx.frames_get(1, 0)) == want_bytes(cam, rows)    # the neighbour is untouched


def test_rows_cameras_arena_and_keep_twice(ctx):
    rng = np.random.default_rng(50)
    ctx.frames_reset(CT2, arena_capacity=4096)                           # 1,024 words, 64 rows: both arenas reallocate on the way
    frames = {f: [PR.make_camera(rng, n, "mixed", with_rows=wr) for n, wr in spec]
              for f, spec in {0: ((300, True), (0, True)), 1: ((520, False), (130, True)), 2: ((257, True), (256, False))}.items()}
    for f, cams in frames.items():
        put(ctx, f, [c for c, _ in cams], [r for _, r in cams])
    assert ctx.frames_info()["arena_reallocations"] >= 1
    state = {(f, k): frames[f][k] for f in frames for k in range(2)}
    for f, k in ((1, 0), (0, 1), (2, 1), (0, 0), (1, 1), (2, 0), (1, 0), (2, 0)):          # (1, 0) and (2, 0): pruned twice in a row
        cam, rows = state[(f, k)]
        n = len(cam[0])
        keep = rng.permutation(n)[:max(n * 2 // 3, min(n, 1))]
        state[(f, k)] = keep_and_check(ctx, f, k, cam, rows, keep)
        for key, (cam2, rows2) in state.items():                         # every other entry is as it was
            assert entry_bytes(ctx.frames_get(*key)) == want_bytes(cam2, rows2), (f, k, key)
    # the arguments that are refused change nothing
    cam, rows = state[(1, 0)]
    before = snapshot(ctx, 1)
    for bad in ([-1], [len(cam[0])], [0, 1, 10 ** 6]):
        with pytest.raises(api.VeloError, match="keep_idx"):
            ctx.frames_keep(1, 0, bad)
    with pytest.raises(api.VeloError, match="frame 7, camera 0 has not been put"):
        ctx.frames_keep(7, 0, [0])
    assert snapshot(ctx, 1) == before
    # the pruned entries serve the builds: ids against ids, rows against rows
    cams1, cams2 = [state[(2, 0)][0], state[(1, 1)][0]], [state[(0, 0)][0], state[(1, 1)][0]]
    put(ctx, 3, cams1)
    put(ctx, 4, cams2)
    want, want_n = VR.assemble(cams1, cams2, CT2)
    per_cam, pairs = ctx.build_matches(3, 4)
    assert ctx.get_visual().tobytes() == want.tobytes() and per_cam.tolist() == want_n.tolist() and want_n[1] > 50


# ---- the registration-driven prune ------------------------------------------------------------------------------------------------
def frames_from_records(rec, seed):
    """frame 1 (frame1) and frame 0 (frame2), 2 cameras, whose id join gives the records of synth.stereo_matches back: shuffled
    keypoint order, distinct ids, and keypoints on either side that match nothing"""
    rng = np.random.default_rng(seed)
    m = api.matches_from_dict(rec)
    sides = {0: [], 1: []}
    for cam in range(2):
        r = m[m["cam"] == cam]
        n, extra = len(r), 9
        for fr, kp, p3, d, lo in ((1, r["p2_1"], r["p3_1"], r["d1"], 10000), (0, r["p2_2"], r["p3_2"], r["d2"], 20000)):
            ids = np.r_[1000 * cam + np.arange(n), lo + 100 * cam + np.arange(extra)].astype(np.int32)   # distinct per camera
            kps = np.vstack([kp, rng.normal(size=(extra, 2)) * .2]).astype(np.float32)
            with_depth = np.flatnonzero(np.r_[d != 0, np.zeros(extra, bool)])
            has = np.full(n + extra, -1, dtype=np.int32)
            slot = rng.permutation(len(with_depth))
            has[with_depth] = slot
            cloud = np.zeros((len(with_depth), 3), dtype=np.float32)
            cloud[slot] = p3[with_depth]
            perm = rng.permutation(n + extra)
            sides[fr].append((ids[perm], kps[perm], has[perm], cloud))
    return sides


@pytest.fixture(scope="module")
def case():
    d = synth.scan_pair(16, 128)
    sides = frames_from_records(synth.stereo_matches(60, mix="all"), 4)
    assert all(len(c[0]) == 69 for f in (0, 1) for c in sides[f])
    rng = np.random.default_rng(61)
    rows1, rows0 = LP.near_rows(rng, sides[1], sides[0])
    return dict(d=d, f1=sides[1], f0=sides[0], rows1=rows1, rows0=rows0, ct=synth.CAM_TRANS[:2].astype(np.float32))


def loaded(case, n_cams=2, with_rows=True, **kw):
    """a context with the scan pair loaded and frames 1 and 0 put (their first n_cams cameras)"""
    c = api.Context(0, icp_skip=2, **kw)
    c.set_target(case["d"]["tgt_xyz"], case["d"]["tgt_off"])
    c.set_source(case["d"]["src_xyz"], case["d"]["src_off"])
    c.frames_reset(case["ct"][:n_cams])
    put(c, 1, case["f1"][:n_cams], case["rows1"] if with_rows else None)
    put(c, 0, case["f0"][:n_cams], case["rows0"] if with_rows else None)
    return c


def result(x, T, s):
    return np.asarray(x).tobytes() + np.asarray(T).tobytes(), bytes(s)


def successor(rng, pruned, pruned_rows):
    """frame 2 of the walk: per camera 40 keypoints, most of whose ids the pruned frame 1 holds, with rows near that frame's rows"""
    cams, rows = [], []
    for (ids, _, _, _), pr in zip(pruned, pruned_rows):
        cam = VR.random_camera(rng, 40, np.r_[ids, 30000 + np.arange(25)])
        where = {int(i): k for k, i in enumerate(ids)}
        q = LP.rand_rows(rng, 40)
        hit = [k for k, i in enumerate(cam[0]) if int(i) in where]
        q[hit] = LP.flip_bits(rng, pr[[where[int(cam[0][k])] for k in hit]], rng.integers(0, 30, len(hit)))
        cams.append(cam)
        rows.append(q)
    return cams, rows


def test_registration_driven_prune(case):
    lidar = loaded(case)
    lidar_before = result(*lidar.frame_to_frame(case["d"]["x0"]))[0]
    c = loaded(case)
    per_cam, _ = c.build_matches(1, 0)
    assert per_cam.tolist() == [60, 60]
    c.frame_to_frame(case["d"]["x0"])
    gm = c.good_matches()
    visual_before = c.get_visual().tobytes()
    kept, n_wd = c.frames_prune(1)
    pruned, pruned_rows = [], []
    for cam in range(2):
        first = gm["point1"][gm["cam"] == cam]
        print(f"camera {cam}: {len(first)} good matches, {len(np.unique(first))} distinct point1 of 69 keypoints")
        assert kept[cam].tolist() == np.unique(first).tolist()
        assert 0 < len(kept[cam]) < 69
        want = PR.prune_literal(case["f1"][cam], case["rows1"][cam], first)
        assert PR.same(want, PR.prune_vectorised(case["f1"][cam], case["rows1"][cam], first))
        assert entry_bytes(c.frames_get(1, cam)) == want_bytes(want[0], want[1]) and n_wd[cam] == len(want[0][3])
        pruned.append(want[0])
        pruned_rows.append(want[1])
    assert any(len(gm["point1"][gm["cam"] == cam]) > len(kept[cam]) for cam in range(2))       # a keypoint with two blocks stays once
    assert c.frames_count(1)[0].tolist() == [len(k) for k in kept]
    assert c.good_matches().tobytes() == gm.tobytes() and c.get_visual().tobytes() == visual_before      # both keep the OLD indices
    for cam in range(2):                                                 # frame 0 is untouched
        assert entry_bytes(c.frames_get(0, cam)) == want_bytes(case["f0"][cam], case["rows0"][cam])
    # the pruned frame is frame2 of the next frame's edges: by id, and by descriptor
    f2, rows2 = successor(np.random.default_rng(62), pruned, pruned_rows)
    put(c, 2, f2, rows2)
    want, want_n = VR.assemble(f2, pruned, case["ct"])
    per_cam, pairs = c.build_matches(2, 1)
    assert c.get_visual().tobytes() == want.tobytes() and per_cam.tolist() == want_n.tolist() and min(want_n) >= 5
    want, want_n, _ = LP.assemble(f2, pruned, rows2, pruned_rows, case["ct"])
    per_cam, pairs = c.build_matches_desc(2, 1)
    assert c.get_visual().tobytes() == want.tobytes() and per_cam.tolist() == want_n.tolist() and min(want_n) >= 5
    assert pairs.tolist() == LP.pairs_of(want).tolist()
    # a LiDAR-only registration is what it was: on the pruned context and on one that never built matches
    c.set_visual(None)
    assert result(*c.frame_to_frame(case["d"]["x0"]))[0] == lidar_before
    assert result(*lidar.frame_to_frame(case["d"]["x0"]))[0] == lidar_before
    c.close()
    lidar.close()


def test_every_refusal_changes_nothing(case):
    fresh = api.Context(0)
    with pytest.raises(api.VeloError, match="velo_frames_reset has not run"):
        fresh.frames_prune(1)
    fresh.close()
    c = loaded(case)
    x0 = case["d"]["x0"]

    def refused(frame, why):
        before = snapshot(c, frame), snapshot(c, 0), c.get_visual().tobytes(), c.good_matches().tobytes()
        with pytest.raises(api.VeloError, match=why):
            c.frames_prune(frame)
        assert (snapshot(c, frame), snapshot(c, 0), c.get_visual().tobytes(), c.good_matches().tobytes()) == before

    refused(1, "not built with frame 1")                                 # nothing built yet
    c.frames_put(5, 0, *case["f1"][0])
    refused(5, "frame 5, camera 1 has not been put")                     # a camera of the frame never put
    c.build_matches(1, 0)
    refused(1, "no registration or velo_build_visual")                   # the flags are not valid
    c.frame_to_frame(x0)
    refused(0, "not built with frame 0")                                 # frame2 of the build is not frame1
    c.set_query_shard(1, 2)
    refused(1, "slice of the visual set")                                # a sharded rank
    c.set_query_shard(0, 1)
    c.frames_put(1, 1, *case["f1"][1])                                   # the frame changed under the visual set: put ...
    refused(1, "camera 1 has changed")
    c.build_matches(1, 0)
    c.frame_to_frame(x0)
    c.frames_keep(1, 0, np.arange(69))                                   # ... keep (even of everything) ...
    refused(1, "camera 0 has changed")
    c.build_matches(1, 0)
    c.frame_to_frame(x0)
    c.frames_drop(1)                                                     # ... drop and put again
    put(c, 1, case["f1"], case["rows1"])
    refused(1, "has changed")
    c.build_matches(1, 0)
    c.frame_to_frame(x0)
    c.set_visual(c.get_visual())                                         # the same records, but the caller's
    refused(1, "not built with frame 1")
    c.build_matches_desc(1, 0)
    c.build_visual(x0, 1)                                                # velo_build_visual validates the flags as a registration does
    gm = c.good_matches()
    kept, _ = c.frames_prune(1)
    assert [k.tolist() for k in kept] == [np.unique(gm["point1"][gm["cam"] == cam]).tolist() for cam in range(2)]
    refused(1, "has changed")                                            # a second prune on the same visual set
    c.build_matches(1, 0)
    c.frame_to_frame(x0)
    c.frames_reset(case["ct"])
    with pytest.raises(api.VeloError, match="has not been put"):
        c.frames_prune(1)
    put(c, 1, case["f1"])
    put(c, 0, case["f0"])
    refused(1, "not built with frame 1")                                 # the reset forgot the build
    c.close()


def test_batch_equals_single_calls(case):
    """3 contexts: 2 cameras with rows, 1 camera whose visual set is empty (nothing kept), 1 camera without rows; batch and single
    calls alternate, twins driven by single calls only give the expected bytes"""
    x0 = case["d"]["x0"]
    rng = np.random.default_rng(70)
    lone = [VR.random_camera(rng, 300, np.arange(50000, 52000))]         # shares no id with frame 0

    def group():
        return [loaded(case), loaded(case, n_cams=1), loaded(case, n_cams=1, with_rows=False)]
    batch, twins = group(), group()
    n_kept_seen = np.zeros(3, dtype=np.int64)
    for step in range(3):
        for g in (batch, twins):
            put(g[0], 1, case["f1"], case["rows1"])
            put(g[1], 1, lone, [LP.rand_rows(np.random.default_rng(71), 300)])
            put(g[2], 1, case["f1"][:1])
            for k, c in enumerate(g):
                c.build_matches(1, 0)
                if k == 1:
                    assert c.build_visual(x0, 1) == 0
                else:
                    c.frame_to_frame(x0)
        want = [api.frames_prune_batch([c], [1], raw=True) for c in twins]
        if step % 2 == 0:
            got = api.frames_prune_batch(batch, [1, 1, 1], raw=True)
            got = [tuple(a[k:k + 1] for a in got) for k in range(3)]
        else:
            got = [api.frames_prune_batch([c], [1], raw=True) for c in batch]
        for k in range(3):
            for a, b in zip(got[k], want[k]):
                w = min(a.shape[-1], b.shape[-1])
                assert a[..., :w].tobytes() == b[..., :w].tobytes() and not a[..., w:].any() and not b[..., w:].any(), (step, k)
            assert snapshot(batch[k], 1) == snapshot(twins[k], 1) and snapshot(batch[k], 0) == snapshot(twins[k], 0), (step, k)
            assert batch[k].good_matches().tobytes() == twins[k].good_matches().tobytes()
            n_kept_seen[k] += want[k][3][0]
        assert want[1][3][0] == 0 and snapshot(batch[1], 1)[1] == [0]
        gm = twins[0].good_matches()
        assert want[0][0][0, :2].tolist() == [len(np.unique(gm["point1"][gm["cam"] == cam])) for cam in range(2)]
    assert n_kept_seen[0] > 30 and n_kept_seen[1] == 0 and n_kept_seen[2] > 15
    for c in batch + twins:
        c.close()
