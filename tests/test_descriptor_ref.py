"""CPU: the descriptor-matching checker (descriptor_ref.match) equals the literal transcription of velo.h:527-549 (match_scalar) on small
crafted sets -- ties, the threshold's edges, the extremes of the distance, empty sets -- and the scalar form gives the hand-derived
answers of the crafted cases."""
import numpy as np
import pytest

import descriptor_ref as R


def rows_with_bits(counts, seed=0):
    """row i has counts[i] set bits (at random positions): distance to the zero row = counts[i]"""
    rng = np.random.default_rng(seed)
    out = np.zeros((len(counts), 512), np.uint8)
    for i, c in enumerate(counts):
        out[i, rng.choice(512, size=c, replace=False)] = 1
    return np.packbits(out, axis=1, bitorder="little")


def same(a, b):
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.array_equal(a[3], b[3]), (a, b)


def test_random_sets_equal_the_scalar_transcription():
    rng = np.random.default_rng(1)
    for nq, nt in ((1, 1), (7, 5), (13, 31), (40, 3)):
        q = rng.integers(0, 256, (nq, 64), dtype=np.uint8)
        t = rng.integers(0, 256, (nt, 64), dtype=np.uint8)
        k = min(nq, nt) // 2
        t[:k] = q[:k]                                            # a few exact matches: min_dist 0
        same(R.match(q, t), R.match_scalar(q, t))


def test_ties_take_the_lowest_train_index():
    q = np.zeros((3, 64), np.uint8)
    t = rows_with_bits([5, 3, 7, 3, 3], seed=2)                 # rows 1, 3, 4 tie at distance 3
    for f in (R.match, R.match_scalar):
        idx, dist, md, pairs = f(q, t)
        assert list(idx) == [1, 1, 1] and list(dist) == [3, 3, 3] and md == 3
        assert pairs.tolist() == [[0, 1], [1, 1], [2, 1]]
    same(R.match(q, t), R.match_scalar(q, t))


def test_all_equal_train_rows():
    rng = np.random.default_rng(3)
    q = rng.integers(0, 256, (6, 64), dtype=np.uint8)
    t = np.repeat(rng.integers(0, 256, (1, 64), dtype=np.uint8), 9, axis=0)
    res = R.match_scalar(q, t)
    assert (res[0] == 0).all()
    same(R.match(q, t), res)


def test_threshold_edges():
    # min_dist 10: the threshold is max(15, 29) = 29 -- distance 29 kept (<=), 30 dropped
    z = np.zeros((1, 64), np.uint8)
    rows = rows_with_bits([10, 29, 30], seed=9)
    for f in (R.match, R.match_scalar):
        idx, dist, md, pairs = f(rows, z)
        assert list(dist) == [10, 29, 30] and md == 10
        assert pairs.tolist() == [[0, 0], [1, 0]]
    # min_dist 29: 1.5 * 29 = 43.5 takes over -- 43 kept, 44 dropped
    rows = rows_with_bits([29, 43, 44, 30], seed=6)
    for f in (R.match, R.match_scalar):
        idx, dist, md, pairs = f(rows, z)
        assert md == 29 and pairs[:, 0].tolist() == [0, 1, 3]
    same(R.match(rows, z), R.match_scalar(rows, z))


def test_exactly_one_and_a_half_min_dist():
    # min_dist 40: threshold 60; 60 kept, 61 dropped
    rows = rows_with_bits([40, 60, 61, 59], seed=10)
    z = np.zeros((1, 64), np.uint8)
    for f in (R.match, R.match_scalar):
        idx, dist, md, pairs = f(rows, z)
        assert md == 40 and list(dist) == [40, 60, 61, 59]
        assert pairs[:, 0].tolist() == [0, 1, 3]


def test_min_dist_zero_keeps_up_to_match_thresh():
    rows = rows_with_bits([0, 29, 30, 1], seed=11)
    z = np.zeros((1, 64), np.uint8)
    for f in (R.match, R.match_scalar):
        idx, dist, md, pairs = f(rows, z)
        assert md == 0 and pairs[:, 0].tolist() == [0, 1, 3]


def test_distance_extremes():
    z = np.zeros((1, 64), np.uint8)
    o = np.full((1, 64), 0xFF, np.uint8)
    for f in (R.match, R.match_scalar):
        idx, dist, md, pairs = f(z, o)
        assert list(dist) == [512] and md == 512 and pairs.tolist() == [[0, 0]]      # 512 <= 1.5 * 512
        idx, dist, md, pairs = f(np.concatenate([z, o]), np.concatenate([o, z]))
        assert list(idx) == [1, 0] and list(dist) == [0, 0] and md == 0


@pytest.mark.parametrize("nq,nt", [(0, 5), (5, 0), (0, 0)])
def test_empty_sets(nq, nt):
    rng = np.random.default_rng(12)
    q = rng.integers(0, 256, (nq, 64), dtype=np.uint8)
    t = rng.integers(0, 256, (nt, 64), dtype=np.uint8)
    res = R.match_scalar(q, t)
    assert res[2] == -1 and len(res[3]) == 0 and (res[0] == -1).all() and len(res[0]) == nq
    same(R.match(q, t), res)


def test_one_row():
    rng = np.random.default_rng(13)
    q = rng.integers(0, 256, (1, 64), dtype=np.uint8)
    t = rng.integers(0, 256, (1, 64), dtype=np.uint8)
    res = R.match_scalar(q, t)
    assert res[0].tolist() == [0] and res[3].tolist() == [[0, 0]]      # a single match is its own min_dist: always kept
    same(R.match(q, t), res)


def test_chunked_form_across_chunk_edges():
    rng = np.random.default_rng(14)
    q = rng.integers(0, 256, (70, 64), dtype=np.uint8)
    t = rng.integers(0, 256, (23, 64), dtype=np.uint8)
    full = R.match(q, t, chunk=4096)
    for chunk in (1, 7, 64):
        same(R.match(q, t, chunk=chunk), full)
    same(full, R.match_scalar(q, t))
