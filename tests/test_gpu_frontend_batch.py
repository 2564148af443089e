"""GPU: the visual front end of several contexts in one call each (velo_set_images_batch / velo_track_features_batch /
velo_detect_features_batch).  The contract: every stored level, every output byte and every context's state equal what the
single-context entries give when each context's share is handed to them in the same order -- ARRAY-EQUAL / FLOAT-BIT-EQUAL, nothing
left out of a comparison -- and, for two contexts of each case, what the numpy restatements (tests/lk_ref.py, tests/gftt_ref.py)
give.  Covered: 8 contexts of 1226 x 370; units that need very different numbers of selection passes in one call; four image sizes in
one call; interleaved / empty / unnamed job lists; 32 contexts and more cameras than one launch set carries; batch and single calls
mixed over frames; registrations unchanged by batch front-end calls."""
import os

import numpy as np
import pytest

import gftt_ref as G
import lk_ref as R
import velo_amd  # noqa: F401
from velo_amd import api, synth

pytestmark = pytest.mark.gpu
W, H = 1226, 370
SIZES = [(1226, 370), (1241, 376), (1242, 375), (641, 203)]
N8 = 8


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bytes(a, b):
    """nested lists / tuples of arrays, compared byte for byte"""
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same_bytes(x, y) for x, y in zip(a, b))
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def levels_of(c, previous):
    """every stored level of every camera of one slot: {(cam, level, kind): array}"""
    out = {}
    for cam in range(2):
        for lev in range(c.image_levels(previous=previous)):
            for kind in ("img", "dx", "dy"):
                out[(cam, lev, kind)] = c.get_image_level(cam, lev, kind, previous=previous)[0]
    return out


def assert_same_images(a, b, what=""):
    for previous in (True, False):
        la, lb = levels_of(a, previous), levels_of(b, previous)
        assert la.keys() == lb.keys(), (what, previous)
        for k in la:
            assert np.array_equal(la[k], lb[k]), (what, previous, k)


def close_all(ctxs):
    for c in ctxs:
        c.close()


def split_jobs(jobs, n_ctx):
    """per context the (position in the batch list, single-context job) pairs, in the batch list's relative order"""
    per = [[] for _ in range(n_ctx)]
    for j, job in enumerate(jobs):
        per[job[0]].append((j, tuple(job[1:])))
    return per


def track_like_single(singles, jobs, **params):
    """the batch job list answered by one single-context call per context"""
    res = ([None] * len(jobs), [None] * len(jobs), [None] * len(jobs))
    for i, mine in enumerate(split_jobs(jobs, len(singles))):
        if not mine:
            continue
        got = singles[i].track_features([job for _, job in mine], **params)
        for k, (j, _) in enumerate(mine):
            for r in range(3):
                res[r][j] = got[r][k]
    return res


def detect_like_single(singles, jobs, **params):
    res, counts = [None] * len(jobs), np.zeros((len(jobs), 3), np.int32)
    for i, mine in enumerate(split_jobs(jobs, len(singles))):
        if not mine:
            continue
        got, cn = singles[i].detect_features([job for _, job in mine], return_counts=True, **params)
        for k, (j, _) in enumerate(mine):
            res[j], counts[j] = got[k], cn[k]
    return res, counts


@pytest.fixture(scope="module")
def frames8():
    return [synth.tracking_frames(W, H, seed=100 + i) for i in range(N8)]


@pytest.fixture(scope="module")
def fleet(hip_lib, frames8):
    """8 contexts fed by two batch uploads, and 8 fed by velo_set_images"""
    batch = [api.Context(0) for _ in range(N8)]
    single = [api.Context(0) for _ in range(N8)]
    api.set_images_batch(batch, [fr["prev"] for fr in frames8])
    api.set_images_batch(batch, [fr["next"] for fr in frames8])
    for c, fr in zip(single, frames8):
        c.set_images(fr["prev"])
        c.set_images(fr["next"])
    yield dict(batch=batch, single=single)
    close_all(batch + single)


def test_set_images_batch_8_contexts_every_level(fleet, frames8):
    for i in range(N8):
        assert_same_images(fleet["batch"][i], fleet["single"][i], i)
    for i in (1, 6):                                           # and against the restatement directly
        for previous, key in ((True, "prev"), (False, "next")):
            got = levels_of(fleet["batch"][i], previous)
            for cam in range(2):
                pyr = R.build_pyramid(frames8[i][key][cam])
                assert len(pyr) == fleet["batch"][i].image_levels(previous=previous) == 7
                for lev, L in enumerate(pyr):
                    for kind in ("img", "dx", "dy"):
                        assert np.array_equal(got[(cam, lev, kind)], L[kind]), (i, previous, cam, lev, kind)


def track_jobs8(n=3000):
    jobs = []
    for i in range(N8):
        pts = [synth.tracking_points(n, seed=200 + 2 * i + c) for c in range(2)]
        jobs += [(i, pc, cc, pts[pc]) for cc in range(2) for pc in range(2)]        # main.cpp:222-235: 4 jobs per frame
    return jobs


@pytest.mark.parametrize("window", [21, 5, 31])
def test_track_batch_8_contexts_equal_8_single_calls(fleet, frames8, window):
    jobs = track_jobs8()
    got = api.track_features_batch(fleet["batch"], jobs, window=window)
    want = track_like_single(fleet["single"], jobs, window=window)
    assert same_bytes(got, want)
    assert [len(g) for g in got[0]] == [3000] * (4 * N8) and all(0 < g.sum() < 3000 for g in got[2])
    if window != 21:
        return
    for i in (2, 5):                                           # the restatement needs ~1.7 s per context: two of the eight
        P = [R.build_pyramid(im) for im in frames8[i]["prev"]]
        N = [R.build_pyramid(im) for im in frames8[i]["next"]]
        for j, (ci, pc, cc, xy) in enumerate(jobs):
            if ci != i:
                continue
            ref = R.track_job(P[pc], N[cc], xy)
            assert np.array_equal(bits(got[0][j]), bits(ref[0])), (i, j)
            assert np.array_equal(got[1][j], ref[1]) and np.array_equal(got[2][j], ref[2]), (i, j)


@pytest.mark.parametrize("params", [dict(), dict(min_distance=5.0)])
def test_detect_batch_8_contexts_equal_8_single_calls(fleet, frames8, params):
    jobs = [(i, cam, synth.tracking_points(1500, seed=300 + 2 * i + cam)) for i in range(N8) for cam in range(2)]
    got, counts = api.detect_features_batch(fleet["batch"], jobs, return_counts=True, **params)
    want, wcounts = detect_like_single(fleet["single"], jobs, **params)
    assert np.array_equal(counts, wcounts) and same_bytes(got, want)
    if params:
        assert (counts[:, 0] == 3000).all()                    # the cap is reached
    else:
        assert (counts[:, 0] < 3000).all() and (counts[:, 1] > 0).all() and (counts[:, 1] < counts[:, 0]).all()
    for i in (0, 7):                                           # and against the restatement directly
        for j, (ci, cam, ex) in enumerate(jobs):
            if ci != i:
                continue
            xy, v, fr, cn = G.detect(frames8[i]["next"][cam], ex, 3000, 0.001, params.get("min_distance", 12.0))
            assert counts[j].tolist() == cn.tolist(), (j, params)
            assert np.array_equal(got[j][0], xy) and np.array_equal(bits(got[j][1]), bits(v)) and np.array_equal(got[j][2], fr), (j, params)
    for _ in range(2):                                         # repeated calls: identical bytes
        again, acounts = api.detect_features_batch(fleet["batch"], jobs, return_counts=True, **params)
        assert np.array_equal(counts, acounts) and same_bytes(got, again)


def test_detect_batch_capacity_below_the_corner_count_and_untouched_tail(fleet):
    jobs = [(i, cam, None) for i in (3, 0, 5) for cam in (1, 0)]
    want, wcounts = detect_like_single(fleet["single"], jobs)
    for cap in (700, 4000):
        xy = np.full((len(jobs), cap, 2), -7.0, np.float32)
        resp = np.full((len(jobs), cap), -7.0, np.float32)
        fr = np.full((len(jobs), cap), 9, np.uint8)
        _, _, _, counts = api.detect_features_batch_raw(fleet["batch"], jobs, cap, xy, resp, fr)
        assert np.array_equal(counts, wcounts)
        for j in range(len(jobs)):
            n = min(int(counts[j, 0]), cap)
            assert (cap == 700) == (counts[j, 0] > cap)
            assert np.array_equal(xy[j, :n], want[j][0][:n]) and np.array_equal(bits(resp[j, :n]), bits(want[j][1][:n]))
            assert np.array_equal(fr[j, :n], want[j][2][:n].astype(np.uint8))
            assert np.all(xy[j, n:] == -7.0) and np.all(resp[j, n:] == -7.0) and np.all(fr[j, n:] == 9)
    _, _, _, counts = api.detect_features_batch_raw(fleet["batch"], jobs, 0)
    assert np.array_equal(counts, wcounts)


def test_units_with_very_different_selection_lengths_in_one_call(hip_lib, frames8):
    """identical tiles (thousands of ties), the contrast ramp (a dependency chain per row), a flat image (no corner) and a normal
    frame, each in a context of its own, in the same launches"""
    normal = frames8[0]["next"]
    imgs = [[synth.detect_tiles(), normal[0]], [synth.detect_ramp(), normal[1]], [np.full((H, W), 128, np.uint8), normal[0]], normal]
    batch = [api.Context(0) for _ in imgs]
    single = [api.Context(0) for _ in imgs]
    try:
        api.set_images_batch(batch, imgs)
        for c, im in zip(single, imgs):
            c.set_images(im)
        ex = synth.tracking_points(500, seed=12)
        jobs = [(i, cam, ex) for i in range(4) for cam in range(2)]
        for params in (dict(), dict(max_corners=0, min_distance=5.0)):
            got, counts = api.detect_features_batch(batch, jobs, return_counts=True, **params)
            want, wcounts = detect_like_single(single, jobs, **params)
            assert np.array_equal(counts, wcounts) and same_bytes(got, want), params
            for i in range(3):                                 # the crafted images against the restatement
                xy, v, fr, cn = G.detect(imgs[i][0], ex, params.get("max_corners", 3000), 0.001, params.get("min_distance", 12.0))
                j = 2 * i
                assert counts[j].tolist() == cn.tolist(), (i, params)
                assert np.array_equal(got[j][0], xy) and np.array_equal(bits(got[j][1]), bits(v)) and np.array_equal(got[j][2], fr), (i, params)
        assert counts[0, 2] > 10000 and counts[4].tolist() == [0, 0, 0]
    finally:
        close_all(batch + single)


@pytest.fixture(scope="module")
def mixed(hip_lib):
    """four contexts of four image sizes, batch-fed and single-fed"""
    frames = [synth.tracking_frames(w, h, seed=400 + i) for i, (w, h) in enumerate(SIZES)]
    batch = [api.Context(0) for _ in SIZES]
    single = [api.Context(0) for _ in SIZES]
    api.set_images_batch(batch, [fr["prev"] for fr in frames])
    api.set_images_batch(batch, [fr["next"] for fr in frames])
    for c, fr in zip(single, frames):
        c.set_images(fr["prev"])
        c.set_images(fr["next"])
    yield dict(batch=batch, single=single, frames=frames)
    close_all(batch + single)


def test_mixed_sizes_set_images(mixed):
    for i, (w, h) in enumerate(SIZES):
        assert mixed["batch"][i].current_image_size() == (w, h)
        assert_same_images(mixed["batch"][i], mixed["single"][i], (w, h))
    pyr = R.build_pyramid(mixed["frames"][3]["next"][1])      # the odd small size against the restatement
    got = levels_of(mixed["batch"][3], False)
    assert len(pyr) == mixed["batch"][3].image_levels()
    for lev, L in enumerate(pyr):
        for kind in ("img", "dx", "dy"):
            assert np.array_equal(got[(1, lev, kind)], L[kind]), (lev, kind)


@pytest.mark.parametrize("window", [21, 9, 31])
def test_mixed_sizes_track(mixed, window):
    jobs = []
    for i, (w, h) in enumerate(SIZES):
        pts = synth.tracking_points(900, w, h, seed=410 + i, margin=-6.0)      # some start outside the image
        jobs += [(i, 0, 0, pts), (i, 1, 0, pts[:300]), (i, 0, 1, pts[300:])]
    got = api.track_features_batch(mixed["batch"], jobs, window=window)
    assert same_bytes(got, track_like_single(mixed["single"], jobs, window=window))
    if window == 21:
        i = 3
        P = [R.build_pyramid(im) for im in mixed["frames"][i]["prev"]]
        N = [R.build_pyramid(im) for im in mixed["frames"][i]["next"]]
        for j, (ci, pc, cc, xy) in enumerate(jobs):
            if ci == i:
                ref = R.track_job(P[pc], N[cc], xy)
                assert np.array_equal(bits(got[0][j]), bits(ref[0])) and np.array_equal(got[1][j], ref[1]) and np.array_equal(got[2][j], ref[2]), j


@pytest.mark.parametrize("params", [dict(), dict(min_distance=5.0, max_corners=0)])
def test_mixed_sizes_detect(mixed, params):
    jobs = [(i, cam, synth.tracking_points(600, w, h, seed=420 + i)) for i, (w, h) in enumerate(SIZES) for cam in (1, 0)]
    got, counts = api.detect_features_batch(mixed["batch"], jobs, return_counts=True, **params)
    want, wcounts = detect_like_single(mixed["single"], jobs, **params)
    assert np.array_equal(counts, wcounts) and same_bytes(got, want)
    j = 6                                                      # context 3 (641 x 203), camera 1, against the restatement
    xy, v, fr, cn = G.detect(mixed["frames"][3]["next"][1], jobs[j][2], params.get("max_corners", 3000), 0.001, params.get("min_distance", 12.0))
    assert counts[j].tolist() == cn.tolist() and np.array_equal(got[j][0], xy) and np.array_equal(bits(got[j][1]), bits(v)) and np.array_equal(got[j][2], fr)


def test_job_lists_interleaved_empty_unnamed_and_odd_points(fleet):
    big = synth.tracking_points(3000, seed=21, margin=-5.0)
    odd = synth.tracking_points(64, seed=40)
    odd[[3, 17, 40]] = [[np.nan, 100], [300, np.inf], [-np.inf, np.nan]]
    # contexts 4 and 6 are named by no job; sizes 0 / 1 / 65; contexts interleaved in arbitrary order
    jobs = [(5, 0, 1, big[:0]), (2, 1, 1, big[:1]), (0, 0, 0, big[1:66]), (5, 1, 0, big), (2, 0, 1, big[:0]), (7, 0, 1, odd),
            (0, 1, 1, big[100:165]), (3, 0, 0, odd), (1, 1, 0, big[:1]), (5, 0, 0, big[:65]), (2, 0, 0, big[2000:])]
    got = api.track_features_batch(fleet["batch"], jobs)
    assert same_bytes(got, track_like_single(fleet["single"], jobs))
    assert [len(g) for g in got[0]] == [0, 1, 65, 3000, 0, 64, 65, 64, 1, 65, 1000]
    assert not got[1][5][[3, 17, 40]].any() and not got[2][5][[3, 17, 40]].any()
    only_empty = [(3, 0, 0, big[:0]), (1, 1, 1, big[:0])]
    assert [len(g) for g in api.track_features_batch(fleet["batch"], only_empty)[0]] == [0, 0]
    assert api.track_features_batch(fleet["batch"], []) == ([], [], [])
    out = np.array([[-3.0, 5.0], [np.nan, 7.0], [W, 9.0], [np.inf, -np.inf], [50.0, H]], np.float32)
    djobs = [(6, 1, big[:500]), (1, 0, None), (6, 0, np.concatenate([out, big[:50]])), (1, 0, big[:1]), (4, 1, big[:65]), (6, 1, big[:0]),
             (1, 1, big), (6, 1, None)]
    dgot, dcounts = api.detect_features_batch(fleet["batch"], djobs, return_counts=True)
    dwant, dwcounts = detect_like_single(fleet["single"], djobs)
    assert np.array_equal(dcounts, dwcounts) and same_bytes(dgot, dwant)
    assert api.detect_features_batch(fleet["batch"], []) == []


def test_one_context_is_the_single_context_entry(fleet):
    pts = synth.tracking_points(700, seed=33)
    tjobs = [(0, 0, 1, pts), (0, 1, 1, pts[:65])]
    assert same_bytes(api.track_features_batch([fleet["batch"][4]], tjobs), fleet["single"][4].track_features([j[1:] for j in tjobs]))
    djobs = [(0, 1, pts), (0, 0, None)]
    got, counts = api.detect_features_batch([fleet["batch"][4]], djobs, return_counts=True)
    want, wcounts = fleet["single"][4].detect_features([j[1:] for j in djobs], return_counts=True)
    assert np.array_equal(counts, wcounts) and same_bytes(got, want)
    one, ref = api.Context(0), api.Context(0)
    try:
        imgs = synth.tracking_frames(641, 203, seed=9)["next"]
        api.set_images_batch([one], [imgs])
        ref.set_images(imgs)
        with pytest.raises(api.VeloError):
            one.get_image_level(0, 0, previous=True)           # one frame only: no previous images yet
        for k, v in levels_of(ref, False).items():
            assert np.array_equal(one.get_image_level(k[0], k[1], k[2])[0], v), k
    finally:
        close_all([one, ref])


def small_fleet(n, n_cams, seed0):
    w, h = 641, 203
    frames = [synth.tracking_frames(w, h, seed=seed0 + i) for i in range(n)]
    extra = [[synth.render_texture(w, h, seed=seed0 + 50 + 7 * i + k, n_blobs=300) for k in range(n_cams - 2)] for i in range(n)]
    prev = [fr["prev"] + [e[::-1].copy() for e in ex] for fr, ex in zip(frames, extra)]
    nxt = [fr["next"] + ex for fr, ex in zip(frames, extra)]
    batch = [api.Context(0) for _ in range(n)]
    single = [api.Context(0) for _ in range(n)]
    api.set_images_batch(batch, prev)
    api.set_images_batch(batch, nxt)
    for c, a, b in zip(single, prev, nxt):
        c.set_images(a)
        c.set_images(b)
    return batch, single


@pytest.mark.parametrize("n_cams", [2, 3])
def test_32_contexts_in_one_call(hip_lib, n_cams):
    """32 contexts of 641 x 203; with 3 cameras each the call names 96 cameras, more than one detection launch set carries"""
    batch, single = small_fleet(32, n_cams, 500)
    try:
        for i in (0, 13, 31):
            assert_same_images(batch[i], single[i], i)
        pts = synth.tracking_points(300, 641, 203, seed=77)
        tjobs = [(i, i % n_cams, (i + 1) % n_cams, pts[(i % 7) * 10:]) for i in range(31, -1, -1)] + [(i, 0, 0, pts[:65]) for i in range(32)]
        assert same_bytes(api.track_features_batch(batch, tjobs), track_like_single(single, tjobs))
        djobs = [(i, cam, pts[:100 + i]) for cam in range(n_cams) for i in range(32)]
        got, counts = api.detect_features_batch(batch, djobs, return_counts=True)
        want, wcounts = detect_like_single(single, djobs)
        assert np.array_equal(counts, wcounts) and same_bytes(got, want)
        assert (counts[:, 0] > 0).all()
    finally:
        close_all(batch + single)


def test_refused_calls_touch_nothing(fleet):
    pts = synth.tracking_points(200, seed=3)
    with pytest.raises(api.VeloError, match="cameras"):
        api.track_features_batch(fleet["batch"], [(0, 0, 1, pts), (3, 0, 2, pts)])        # two cameras were uploaded
    with pytest.raises(api.VeloError, match="camera 2 outside"):
        api.detect_features_batch(fleet["batch"], [(1, 0, pts), (6, 2, None)])
    with pytest.raises(api.VeloError, match="same context"):
        api.detect_features_batch([fleet["batch"][0], fleet["batch"][1], fleet["batch"][0]], [(0, 0, None)])
    with pytest.raises(api.VeloError, match="context index 8"):
        api.track_features_batch(fleet["batch"], [(8, 0, 0, pts)])
    empty = api.Context(0)
    try:
        with pytest.raises(api.VeloError, match="context 1"):
            api.track_features_batch([fleet["batch"][0], empty], [(0, 0, 0, pts), (1, 0, 0, pts)])
        with pytest.raises(api.VeloError, match="context 1: no current images"):
            api.detect_features_batch([fleet["batch"][0], empty], [(1, 0, None)])
        # a context without images that no job names is no error
        got = api.track_features_batch([fleet["batch"][0], empty], [(0, 0, 1, pts)])
        assert same_bytes(got, fleet["single"][0].track_features([(0, 1, pts)]))
    finally:
        empty.close()
    tjobs = [(0, 0, 1, pts), (3, 0, 1, pts)]
    assert same_bytes(api.track_features_batch(fleet["batch"], tjobs), track_like_single(fleet["single"], tjobs))
    djobs = [(1, 0, pts), (6, 1, None)]
    got, counts = api.detect_features_batch(fleet["batch"], djobs, return_counts=True)
    want, wcounts = detect_like_single(fleet["single"], djobs)
    assert np.array_equal(counts, wcounts) and same_bytes(got, want)


def test_batch_and_single_calls_mixed_over_frames(hip_lib):
    """three contexts over four frames: uploads alternate between the batch and the single entry, one context is left out of a batch
    upload and keeps its images; after every frame all slots, tracking and detection equal a context fed by velo_set_images only"""
    w, h = 641, 203
    seq = [[synth.tracking_frames(w, h, seed=600 + 10 * i + f)["next"] for f in range(4)] for i in range(3)]
    mix = [api.Context(0) for _ in range(3)]
    ref = [api.Context(0) for _ in range(3)]
    pts = synth.tracking_points(400, w, h, seed=8)
    try:
        for c, s in zip(ref, seq):
            c.set_images(s[0])
        api.set_images_batch(mix, [s[0] for s in seq])                     # frame 0: batch
        for c, s in zip(mix + ref, seq + seq):                             # frame 1: single
            c.set_images(s[1])
        for i in range(3):
            assert_same_images(mix[i], ref[i], ("frame 1", i))
        tjobs = [(2, 0, 1, pts), (0, 1, 0, pts), (1, 0, 0, pts[:65])]
        assert same_bytes(api.track_features_batch(mix, tjobs), track_like_single(ref, tjobs))      # single upload, batch track
        api.set_images_batch([mix[2], mix[0]], [seq[2][2], seq[0][2]])     # frame 2: batch, other order, context 1 left out
        ref[0].set_images(seq[0][2])
        ref[2].set_images(seq[2][2])
        for i in range(3):
            assert_same_images(mix[i], ref[i], ("frame 2", i))
        for i in range(3):                                                 # batch upload, single track / detect
            assert same_bytes(mix[i].track_features([(0, 1, pts)]), ref[i].track_features([(0, 1, pts)]))
            assert same_bytes(mix[i].detect_features([(1, pts)]), ref[i].detect_features([(1, pts)]))
        mix[1].set_images(seq[1][2])                                       # context 1 catches up by a single call
        ref[1].set_images(seq[1][2])
        api.set_images_batch(mix, [s[3] for s in seq])                     # frame 3: batch
        for c, s in zip(ref, seq):
            c.set_images(s[3])
        for i in range(3):
            assert_same_images(mix[i], ref[i], ("frame 3", i))
        djobs = [(1, 0, pts), (0, 1, None), (2, 1, pts)]
        got, counts = api.detect_features_batch(mix, djobs, return_counts=True)
        want, wcounts = detect_like_single(ref, djobs)
        assert np.array_equal(counts, wcounts) and same_bytes(got, want)
        assert same_bytes(api.track_features_batch(mix, tjobs), track_like_single(ref, tjobs))
    finally:
        close_all(mix + ref)


def test_registration_unchanged_by_batch_front_end_calls(hip_lib):
    m = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "mini_pair.npz")))
    w, h = 641, 203
    frames = [synth.tracking_frames(w, h, seed=700 + i) for i in range(2)]
    pts = synth.tracking_points(300, w, h, seed=5)

    def load(c):
        c.set_target(m["tgt_xyz"], m["tgt_off"])
        c.set_source(m["src_xyz"], m["src_off"])
        c.set_visual(m["matches"])

    def summary(s):
        return (s.n_solves, s.n_assoc_rounds, s.n_queries, s.n_target, s.algorithmic_bytes, s.assoc_bytes,
                [(s.solves[i].lm_iterations, s.solves[i].termination, s.solves[i].evaluations, s.solves[i].initial_cost, s.solves[i].final_cost)
                 for i in range(s.n_solves)])

    plain = api.Context(0, icp_skip=1)
    mixed_ = [api.Context(0, icp_skip=1) for _ in range(2)]
    try:
        load(plain)
        xa, Ta, sa = plain.frame_to_frame(m["x0"])
        api.set_images_batch(mixed_, [fr["prev"] for fr in frames])
        for c in mixed_:
            load(c)
        api.set_images_batch(mixed_, [fr["next"] for fr in frames])
        api.track_features_batch(mixed_, [(1, 0, 1, pts), (0, 0, 0, pts)])
        res = [c.frame_to_frame(m["x0"]) for c in mixed_]
        api.detect_features_batch(mixed_, [(0, 1, pts), (1, 0, None)])
        api.set_images_batch(mixed_[::-1], [fr["prev"] for fr in frames[::-1]])
        res += [c.frame_to_frame(m["x0"]) for c in mixed_]
        xd, Td, sd = plain.frame_to_frame(m["x0"])
    finally:
        close_all([plain] + mixed_)
    for x, T, s in res[:2]:                                    # a context's first registration, and its second
        assert np.array_equal(x, xa) and np.array_equal(T, Ta) and summary(s) == summary(sa)
    for x, T, s in res[2:]:
        assert np.array_equal(x, xd) and np.array_equal(T, Td) and summary(s) == summary(sd)


def test_cxx_batch_adaptors_append_what_the_single_sequence_members_append(tmp_path, hip_lib):
    """include/velo_track_features.hpp setImagesBatch / trackFeaturesFrameBatch and include/velo_detect_features.hpp
    detectFeaturesFrameBatch over three sequences of three image sizes: per sequence and camera the appended key points, pixel points,
    ids and descriptor rows, after tracking and after detection, and the id counters equal what the single-sequence members give
    (tests/cpp/test_frontend_batch.cpp runs both); sequence 1 also against the restatement's tracking"""
    import struct
    import subprocess
    from test_frontend_batch_cpu import compile_frontend_batch_driver
    from test_track_cpu import K, parse_lists
    exe = compile_frontend_batch_driver(tmp_path)
    sizes = [(320, 160), (300, 170), (257, 129)]
    n_pts, first_id = 30, 7000                              # few enough points that detection finds room for fresh corners
    Ks = [K, (K + np.array([[2, 0, -3], [0, 2, 1.5], [0, 0, 0]], np.float32)).astype(np.float32)]
    Kinv = [np.linalg.inv(k.astype(np.float64)).astype(np.float32) for k in Ks]
    rng = np.random.default_rng(11)
    frames, pts, ids, desc = [], [], [], []
    case = str(tmp_path / "batch.bin")
    with open(case, "wb") as f:
        f.write(struct.pack("iii", len(sizes), 2, first_id))
        for s, (w, h) in enumerate(sizes):
            fr = synth.tracking_frames(w, h, seed=800 + s, disparity=4.5)
            frames.append(fr)
            pts.append([synth.tracking_points(n_pts, w, h, seed=810 + 2 * s + c, margin=-4.0) for c in range(2)])
            ids.append([np.arange(n_pts) + 1000 * s, np.arange(200, 200 + n_pts) + 1000 * s])
            desc.append([rng.integers(0, 256, (n_pts, 64), dtype=np.uint8) for _ in range(2)])
            f.write(struct.pack("ii", w, h))
            for im in fr["prev"] + fr["next"]:
                f.write(np.ascontiguousarray(im).tobytes())
            for c in range(2):
                f.write(Ks[c].tobytes())
                f.write(Kinv[c].tobytes())
            for c in range(2):
                f.write(struct.pack("i", n_pts))
                f.write(pts[s][c].astype(np.float32).tobytes())
                f.write(ids[s][c].astype(np.int32).tobytes())
                f.write(desc[s][c].tobytes())
    out = subprocess.run([exe, case], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    got = parse_lists(out.stdout)
    for stage in ("track", "detect"):
        for suffix in ("_k", "_p", "_id", "_d"):
            a, b = got[f"single_{stage}{suffix}"], got[f"batch_{stage}{suffix}"]
            assert len(a) == len(b) == 2 * len(sizes)
            for i, (x, y) in enumerate(zip(a, b)):
                assert x.shape == y.shape and x.tobytes() == y.tobytes(), (stage, suffix, i)
                assert len(x) > 0, (stage, suffix, i)
    for i in range(2 * len(sizes)):                            # detection appended to what tracking left
        assert len(got["batch_detect_id"][i]) > len(got["batch_track_id"][i]) > 0.5 * n_pts
    assert got["single_counters"][0].tolist() == got["batch_counters"][0].tolist()
    assert all(c > first_id + 10000 * s for s, c in enumerate(got["batch_counters"][0].tolist()))
    s = 1                                                       # one sequence against the restatement: what trackFeaturesFrame appends
    P = [R.build_pyramid(i) for i in frames[s]["prev"]]
    N = [R.build_pyramid(i) for i in frames[s]["next"]]
    for cam in range(2):
        kp_p, kid = [], []
        for pc in range(2):
            nxt, _, kept = R.track_job(P[pc], N[cam], pts[s][pc])
            kp_p += [nxt[i] for i in np.nonzero(kept)[0]]
            kid += [int(ids[s][pc][i]) for i in np.nonzero(kept)[0]]
        assert np.array_equal(got["batch_track_p"][2 * s + cam].view(np.uint32), np.asarray(kp_p, np.float32).reshape(-1, 2).view(np.uint32))
        assert got["batch_track_id"][2 * s + cam].tolist() == kid
