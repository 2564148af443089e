"""Every page-locked staging buffer of the visual side across a context's life.  On ONE context each stage that owns such a buffer is
called small and then at least four times larger, so that the buffer is freed and allocated again between the two calls; the context
is destroyed, a new one is created and the same calls are made again.  Both rounds equal the Python restatements -- compared exactly
as the stage's own GPU test compares -- and are byte-identical to each other.

Staging bytes of the small and the large call (a buffer of b bytes is allocated with b + b / 4 + 4096):
  match_descriptors   8 -> 256 rows: upload 1 KB -> 32 KB; the landing (16 bytes a query) grows only with the third size, 2,048 rows
  set_images          64 x 48 -> 256 x 128, two cameras: 6 KB -> 64 KB of raw pixels
  track / detect      6 -> 700 points; max_corners 50, one job -> 3,000, two jobs: the landing 0.7 KB -> 78 KB
  landmarks           8 ids over frames 0..2, then 700 ids over frames 3..5 (20 bytes an observation, 28 a solved landmark)
  frames              one camera, 8 -> 300 keypoints and rows; the landing of the two builds (8 bytes a pair) grows only with the third
                      size, 3,000 keypoints, and their upload only with the candidate count of match_frames (1 -> 256)"""
import numpy as np
import pytest

import descriptor_ref as DR
import gftt_ref as G
import landmarks_ref as LR
import lk_ref as LK
import loop_ref as LP
import visual_ref as VR
import velo_amd  # noqa: F401
from velo_amd import api, synth
import test_gpu_detect as TD
import test_gpu_landmarks as TL
import test_gpu_loop_matches as TLM
import test_gpu_match as TM
import test_gpu_track as TT
import test_gpu_visual_assembly as TV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    """inputs and restatement results that do not depend on the device, made once for both rounds"""
    rng = np.random.default_rng(31)
    match = []
    for n in (8, 256, 2048):
        t = TM.rand_rows(rng, n)
        q, _ = TM.near_duplicates(rng, t, rng.integers(0, 40, n))
        match.append((q, t, DR.match(q, t)))
    images = []
    for (w, h), n_pts, params in (((64, 48), 6, dict(max_corners=50)), ((256, 128), 700, dict())):
        fr = synth.tracking_frames(w, h, seed=4, flat=False)
        pts = synth.tracking_points(n_pts, w, h, seed=9)
        images.append(dict(fr=fr, prev=[LK.build_pyramid(i) for i in fr["prev"]], next=[LK.build_pyramid(i) for i in fr["next"]],
                           eig=[G.response(i) for i in fr["next"]], pts=pts, params=params))
    small, large = list(range(8)), list(range(100, 800))
    seq = LR.sequence(33, 6, 2, small + large, first_frame={**{i: (0, 3) for i in small}, **{i: (3, 3) for i in large}})
    ct = np.float32([[.1, .2, .3]])
    frames = [LP.random_pair(40 + n, (n,), (n,)) for n in (8, 300, 3000)]
    return dict(match=match, images=images, seq=seq, ct=ct, frames=frames)


def one_round(cases):
    """every stage small, then large, on a fresh context; what the device gave, as bytes"""
    out = []
    c = api.Context(0)
    try:
        for q, t, want in cases["match"]:
            got = c.match_descriptors(q, t)
            TM.check(got, want)
            out += [np.asarray(g).tobytes() for g in got]
        for im in cases["images"]:
            c.set_images(im["fr"]["prev"])
            c.set_images(im["fr"]["next"])
            jobs = [(0, 0, im["pts"]), (1, 1, im["pts"][::2])]
            got = TT.check_jobs(c, im["prev"], im["next"], jobs)
            out += [a.tobytes() for part in got for a in part]
            djobs = [(0, im["pts"])] if im["params"] else [(0, im["pts"]), (1, None)]
            got, counts = TD.check_jobs(c, im["fr"]["next"], im["eig"], djobs, **im["params"])
            out += [a.tobytes() for job in got for a in job] + [counts.tobytes()]
        seq = cases["seq"]
        book = LR.LandmarkBook(2)
        c.landmarks_reset(seq["cam_trans"])
        for f in range(len(seq["poses"])):
            c.landmarks_set_pose(f, seq["poses"][f])
        n_solved = []
        for f in range(len(seq["poses"])):
            TL.book_observe(book, f, seq["frames"][f])
            TL.observe(c, f, seq["frames"][f])
            ids, pts, res = TL.path_a_frame(c, book, seq, f)
            gi, gp, gr = c.landmarks_triangulate(f)
            assert gi.tolist() == list(ids), f
            assert np.array_equal(TL.bits(gp), TL.bits(pts)), f
            assert gr.tobytes() == np.ascontiguousarray(res).tobytes(), f
            out += [gi.tobytes(), gp.tobytes(), gr.tobytes()]
            n_solved.append(len(ids))
        assert 0 < n_solved[2] <= 8 and n_solved[5] >= 4 * 8 and 28 * n_solved[5] > 28 * n_solved[2] + 8192
        ct = cases["ct"]
        c.frames_reset(ct)
        for k, (f1, f2, d1, d2, _) in enumerate(cases["frames"]):
            a, b = 2 * k + 1, 2 * k
            TLM.put(c, a, f1, d1)
            TLM.put(c, b, f2, d2)
            want = TV.check(c, a, b, f1, f2, ct)
            out += [want.tobytes(), c.get_visual().tobytes()]
            want = TLM.check(c, a, b, f1, f2, d1, d2, ct)
            out += [want.tobytes(), c.get_visual().tobytes()]
            cand = [b] * (1 if k == 0 else 256)
            kept, md = c.match_frames(a, cand)
            _, want_n, want_md = LP.assemble(f1, f2, d1, d2, ct)
            assert md.tolist() == [want_md.tolist()] * len(cand) and kept.tolist() == [want_n.tolist()] * len(cand)
            out += [kept.tobytes(), md.tobytes()]
    finally:
        c.close()
    return out


def test_two_context_lives_equal_the_restatements_and_each_other(cases):
    first = one_round(cases)
    second = one_round(cases)
    assert len(first) == len(second) > 60
    assert all(a == b for a, b in zip(first, second))
