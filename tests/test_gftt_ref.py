"""The corner-detection restatement (tests/gftt_ref.py) against independent tools: Sobel and box sums against scipy.ndimage.correlate
(mode="mirror") on int64, the local-maximum test against scipy.ndimage.maximum_filter, the selection in its three forms (literal
scalar transcription with OpenCV's grid, parallel rounds, brute-force O(n^2) greedy) against each other with and without the cap, the
properties of the output, the fresh filter against a literal transcription of velo.h:132-167, and the PARITY BUDGET of the two
choices the restatement makes (exact integer sums instead of OpenCV's float sums; the tie rule), measured on the four frames of
synth.tracking_frames(1226, 370, seed=0) and held with a margin of about 2x."""
import numpy as np
import pytest
from scipy import ndimage as ndi

import gftt_ref as G
import velo_amd  # noqa: F401
from velo_amd import synth

W, H = 1226, 370
KX = np.array([[-1, 0, 1], [-2, 0, 2], [-1, 0, 1]], dtype=np.int64)


@pytest.fixture(scope="module")
def frames():
    fr = synth.tracking_frames(W, H, seed=0)
    return fr["prev"] + fr["next"]


@pytest.fixture(scope="module")
def cand(frames):
    eig = G.response(frames[2])
    return (eig,) + G.candidates(eig, 0.001)


def brute_greedy(xs, ys, md, cap):
    out, px, py = [], np.zeros(0), np.zeros(0)
    md2 = float(md) * float(md)
    for i in range(len(xs)):
        if len(out) and (((px - xs[i]) ** 2 + (py - ys[i]) ** 2) < md2).any():
            continue
        out.append(i)
        px, py = np.append(px, xs[i]), np.append(py, ys[i])
        if cap > 0 and len(out) == cap:
            break
    return np.asarray(out, np.int64)


def test_sobel_and_box_sums_equal_scipy(frames):
    for img in (frames[0], frames[3], synth.render_texture(641, 203, seed=3, n_blobs=200), synth.detect_tiles(97, 33)):
        I = img.astype(np.int64)
        dx, dy = G.sobel(img)
        assert np.array_equal(dx, ndi.correlate(I, KX, mode="mirror")) and np.array_equal(dy, ndi.correlate(I, KX.T, mode="mirror"))
        box = np.ones((3, 3), np.int64)
        for got, prod in zip(G.box_sums(img), (dx * dx, dx * dy, dy * dy)):
            assert np.array_equal(got, ndi.correlate(prod, box, mode="mirror"))
        assert max(abs(int(s.max())) for s in G.box_sums(img)) < 1 << 24
    # the product maps are reflected, not the image: at the outermost ring Sxy differs from sums over a reflected image's derivatives
    p = np.pad(frames[0], 2, mode="reflect")
    dxp, dyp = G.sobel(p)
    wrong = ndi.correlate((dxp * dyp), np.ones((3, 3), np.int64), mode="mirror")[2:-2, 2:-2]
    assert not np.array_equal(wrong, G.box_sums(frames[0])[1]) and np.array_equal(wrong[1:-1, 1:-1], G.box_sums(frames[0])[1][1:-1, 1:-1])


def test_response_is_the_smaller_eigenvalue(frames):
    sxx, sxy, syy = (s.astype(np.float64) for s in G.box_sums(frames[2]))
    s2 = (1.0 / 3060.0) ** 2
    lam = ((sxx + syy) / 2 - np.sqrt(((sxx - syy) / 2) ** 2 + sxy ** 2)) * s2
    e = G.response(frames[2])
    assert e.dtype == np.float32 and np.abs(e - lam).max() <= 4e-7 * lam.max()
    assert G.response(np.full((40, 50), 93, np.uint8)).max() == 0


def test_candidates_equal_maximum_filter(cand):
    eig, xs, ys, v = cand
    thr = G.threshold(eig, 0.001)
    e = np.where(eig > thr, eig, 0).astype(np.float32)
    m = (e != 0) & (e == ndi.maximum_filter(e, size=3, mode="constant", cval=0.0))
    m[0] = m[-1] = False
    m[:, 0] = m[:, -1] = False
    assert np.array_equal(m, G.candidate_mask(eig, 0.001))
    assert len(xs) == m.sum() and np.all(np.diff(v.astype(np.float64)) <= 0)
    same = np.diff(v.astype(np.float64)) == 0
    idx = ys * W + xs
    assert np.all(idx[1:][same] < idx[:-1][same])                      # ties: the higher row-major index first


@pytest.mark.parametrize("md", [1, 3, 5, 8, 12, 12.4, 20])
def test_selection_forms_agree_and_hold_their_properties(cand, md):
    eig, xs, ys, v = cand
    for cap in (0, 3000, 100):
        a = G.select_scalar(xs, ys, W, H, md, cap)
        b, rounds = G.select(xs, ys, W, H, md, cap, return_rounds=True)
        assert np.array_equal(a, b) and np.array_equal(a, brute_greedy(xs, ys, md, cap)), (md, cap)
    full = G.select(xs, ys, W, H, md, 0)
    capped = G.select(xs, ys, W, H, md, 3000)
    assert np.array_equal(capped, full[:3000])                          # the capped list is the prefix
    px, py = xs[full].astype(np.float64), ys[full].astype(np.float64)
    d2 = (px[:, None] - px[None, :]) ** 2 + (py[:, None] - py[None, :]) ** 2 if len(full) <= 4000 else None
    if d2 is not None:
        np.fill_diagonal(d2, np.inf)
        assert d2.min() >= md * md                                      # no two corners closer than min_distance
    acc = np.zeros(len(xs), bool)
    acc[full] = True
    for i in np.nonzero(~acc)[0][::7]:                                  # maximality: a dropped one has an accepted larger key in range
        near = ((xs[full] - xs[i]) ** 2 + (ys[full] - ys[i]) ** 2 < md * md) & (full < i)
        assert near.any(), (md, i)
    assert np.all(np.diff(v[full].astype(np.float64)) <= 0)


def test_reference_parameters_on_seed_0(cand):
    eig, xs, ys, v = cand
    acc, rounds = G.select(xs, ys, W, H, 12, 3000, return_rounds=True)
    assert len(xs) == 11996 and len(acc) == 1793 and rounds == [3196, 737, 111, 9, 0]
    assert [len(G.select(xs, ys, W, H, md, 0)) for md in (8, 5, 3)] == [3586, 7856, 10967]


def test_corners_sit_on_texture_and_a_flat_image_has_none(frames):
    fr = synth.tracking_frames(W, H, seed=0)
    xy, v, n = G.good_features(frames[2])
    for (x0, y0, x1, y1) in fr["flat"]:
        inside = (xy[:, 0] > x0 + 8) & (xy[:, 0] < x1 - 8) & (xy[:, 1] > y0 + 8) & (xy[:, 1] < y1 - 8)
        assert not inside.any()
    assert len(xy) > 1000 and v.min() > G.threshold(G.response(frames[2]), 0.001)
    xy0, v0, n0 = G.good_features(np.full((60, 80), 17, np.uint8))
    assert len(xy0) == 0 and n0 == 0


def test_crafted_images_tie_and_chain():
    t = synth.detect_tiles()
    e = G.response(t)
    xs, ys, v = G.candidates(e, 0.001)
    assert len(xs) > 10000 and len(np.unique(v)) < 100                  # thousands of exactly equal responses
    assert np.array_equal(G.select(xs, ys, W, H, 12, 3000), G.select_scalar(xs, ys, W, H, 12, 3000))
    r = synth.detect_ramp()
    xs, ys, v = G.candidates(G.response(r), 0.001)
    acc, rounds = G.select(xs, ys, W, H, 12, 3000, return_rounds=True)
    assert len(rounds) > 100                                             # far more rounds than the textured frame's 5
    assert np.array_equal(acc, G.select_scalar(xs, ys, W, H, 12, 3000))


def literal_fresh(corners, existing, min_distance, img_width, img_height):
    """velo.h:128-163 transcribed: occupied grid of min_distance cells (col-major), the 3 x 3 cells around a key point"""
    f32 = np.float32
    col_cells, row_cells = img_width // min_distance + 2, img_height // min_distance + 2
    occupied = [[] for _ in range(col_cells * row_cells)]
    for p in existing:
        col, row = int(f32(p[0]) / f32(min_distance)), int(f32(p[1]) / f32(min_distance))
        occupied[col * row_cells + row].append((f32(p[0]), f32(p[1])))
    out = []
    md2 = f32(min_distance * min_distance)
    for kp in corners:
        col, row = int(f32(kp[0]) / f32(min_distance)), int(f32(kp[1]) / f32(min_distance))
        bad = False
        for c in range(max(col - 1, 0), min(col + 1, col_cells - 1) + 1):
            for r in range(max(row - 1, 0), min(row + 1, row_cells - 1) + 1):
                for pp in occupied[c * row_cells + r]:
                    dx, dy = f32(pp[0] - f32(kp[0])), f32(pp[1] - f32(kp[1]))
                    if float(f32(f32(dx * dx) + f32(dy * dy))) < float(md2):
                        bad = True
                        break
                if bad:
                    break
            if bad:
                break
        out.append(not bad)
    return np.asarray(out, bool)


def test_fresh_filter_equals_the_literal_transcription(frames):
    xy, _, _ = G.good_features(frames[2])
    ex = synth.tracking_points(3000, seed=9)
    ex[:40] = xy[:40] + np.array([11.0, 4.7], np.float32)               # around the limit: 11^2 + 4.7^2 = 143.09 < 144
    ex[40:80] = xy[40:80] + np.array([12.0, 0.0], np.float32)           # exactly min_distance away: not < md2
    for md in (12, 5, 20):
        got = G.fresh(xy, ex, md, W, H)
        assert np.array_equal(got, literal_fresh(xy, ex, md, W, H)), md
    assert 0 < G.fresh(xy, ex, 12, W, H).sum() < len(xy)
    out = np.array([[-5.0, 10.0], [np.nan, 3.0], [W + 0.0, 5.0], [np.inf, np.inf]], np.float32)
    assert G.fresh(xy[:50], out, 12, W, H).all() and G.fresh(xy, np.zeros((0, 2)), 12, W, H).all()
    assert not G.fresh(xy, xy, 12, W, H).any()


def test_parity_budget_of_the_summation_order_and_the_tie_rule(frames):
    """Measured (one run of a deterministic computation) on the four frames: OpenCV's float order moves the map by at most 2.26e-7 of
    its maximum and changes 0 of the ~1,800 selected corners per frame; ordering ties by the LOWER index first changes at most 2
    corners (symmetric difference, frame next[1]; 0 on the other three).  Held with a margin of about 2x; for the count that
    measured 0 the bound is one exchanged corner (2 in the symmetric difference)."""
    rels, d_float, d_tie = [], [], []
    for img in frames:
        e, e2 = G.response(img), G.response(img, "opencv_float")
        rels.append(float(np.abs(e2.astype(np.float64) - e).max() / e.max()))
        a = set(map(tuple, G.good_features(img, eig=e)[0]))
        d_float.append(len(a ^ set(map(tuple, G.good_features(img, eig=e2)[0]))))
        d_tie.append(len(a ^ set(map(tuple, G.good_features(img, eig=e, tie="lower")[0]))))
    print("parity budget: rel", rels, "float-order corners", d_float, "tie-rule corners", d_tie)
    assert max(rels) <= 4.6e-7
    assert max(d_float) <= 2
    assert max(d_tie) <= 4
