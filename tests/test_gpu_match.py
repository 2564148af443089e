"""GPU: velo_match_descriptors (matchFeatures, velo.h:499-560) is ARRAY-EQUAL to the numpy restatement (tests/descriptor_ref.py) --
nearest row, distance, min_dist and the kept pairs -- on random, near-duplicate, duplicated and odd-sized sets, empty sets and a mixed
64-job batch; the diagnostics build's XOR + popcount variant equals the int8-MFMA product kernel; a match call between registrations
changes nothing of them; the C++ adaptor gives the same pairs."""
import os
import subprocess

import numpy as np
import pytest

import descriptor_ref as R
import oracle_lib  # noqa: F401  (tests/ on the path)
import velo_amd  # noqa: F401
from velo_amd import api, synth
from test_match_cpu import compile_driver, parse, write_case

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(hip_lib):
    c = api.Context(0)
    yield c
    c.close()


def rand_rows(rng, n):
    return rng.integers(0, 256, (n, 64), dtype=np.uint8)


def near_duplicates(rng, train, flips):
    """queries = train rows (shuffled) with flips[i] random bits flipped: the nearest row is known while flips stay small"""
    pick = rng.permutation(len(train))[:len(flips)]
    bits = np.unpackbits(train[pick], axis=1, bitorder="little")
    for i, f in enumerate(flips):
        bits[i, rng.choice(512, size=int(f), replace=False)] ^= 1
    return np.packbits(bits, axis=1, bitorder="little"), pick


def check(got, want):
    idx, dist, md, pairs = got
    widx, wdist, wmd, wpairs = want
    assert np.array_equal(idx, widx), np.nonzero(idx != widx)
    assert np.array_equal(dist, wdist)
    assert md == wmd
    assert np.array_equal(pairs, wpairs)


def test_random_3000_by_3000(ctx):
    rng = np.random.default_rng(0)
    q, t = rand_rows(rng, 3000), rand_rows(rng, 3000)
    check(ctx.match_descriptors(q, t), R.match(q, t))


def test_near_duplicates_keep_and_drop(ctx):
    rng = np.random.default_rng(1)
    t = rand_rows(rng, 3000)
    q, pick = near_duplicates(rng, t, rng.integers(0, 13, 2000))
    got = ctx.match_descriptors(q, t)
    want = R.match(q, t)
    check(got, want)
    assert (got[0] == pick).all()                          # 12 flips are far below the ~200 bits between random rows
    assert want[2] == 0 and len(want[3]) == len(q)          # min_dist 0: the threshold is match_thresh = 29, which 12 flips pass
    # a stricter threshold makes the filter drop some: max(1.5 * 0, 6)
    got = ctx.match_descriptors(q, t, match_thresh=6.0)
    want = R.match(q, t, match_thresh=6.0)
    check(got, want)
    assert 0 < len(want[3]) < len(q)


def test_duplicated_train_rows_lowest_index_wins(ctx):
    rng = np.random.default_rng(2)
    base = rand_rows(rng, 700)
    t = np.concatenate([base, base, base[::-1], base])     # every row 4 times, far apart in index
    q, _ = near_duplicates(rng, base, rng.integers(0, 5, 500))
    got = ctx.match_descriptors(q, t)
    check(got, R.match(q, t))
    assert (got[0] < 700).all()
    # all-equal train set: train index 0 for every query
    t = np.repeat(base[:1], 1100, axis=0)
    got = ctx.match_descriptors(q, t)
    check(got, R.match(q, t))
    assert (got[0] == 0).all()


@pytest.mark.parametrize("nq,nt", [(1, 1), (15, 15), (33, 33), (2999, 2999), (3001, 3001), (1, 3001), (3001, 15), (20000, 2999),
                                   (2999, 20000)])
def test_sizes_off_every_tile(ctx, nq, nt):
    rng = np.random.default_rng(nq * 7 + nt)
    q, t = rand_rows(rng, nq), rand_rows(rng, nt)
    check(ctx.match_descriptors(q, t), R.match(q, t))


@pytest.mark.parametrize("nq,nt", [(0, 100), (100, 0), (0, 0)])
def test_empty_sets(ctx, nq, nt):
    rng = np.random.default_rng(3)
    q, t = rand_rows(rng, nq), rand_rows(rng, nt)
    got = ctx.match_descriptors(q, t)
    check(got, R.match(q, t))
    assert got[2] == -1 and len(got[3]) == 0 and (got[0] == -1).all()


def mixed_jobs(rng, n_jobs=64):
    """shared query sets (as in a loop-closure batch), mixed sizes, a few empty sets and near duplicates"""
    shared = [rand_rows(rng, 3000), rand_rows(rng, 1234)]
    jobs = []
    for j in range(n_jobs):
        kind = j % 8
        if kind == 0:
            jobs.append((shared[0], rand_rows(rng, int(rng.integers(1, 4000)))))
        elif kind == 1:
            jobs.append((shared[1], rand_rows(rng, int(rng.integers(1, 700)))))
        elif kind == 2:
            t = rand_rows(rng, int(rng.integers(20, 2000)))
            q, _ = near_duplicates(rng, t, rng.integers(0, 13, min(len(t), 300)))
            jobs.append((q, t))
        elif kind == 3:
            jobs.append((rand_rows(rng, int(rng.integers(0, 3))), rand_rows(rng, int(rng.integers(0, 3)))))
        elif kind == 4:
            jobs.append((shared[0], shared[1]))
        else:
            jobs.append((rand_rows(rng, int(rng.integers(1, 3100))), rand_rows(rng, int(rng.integers(1, 3100)))))
    return jobs


def test_batch_of_64_equals_64_single_calls(ctx):
    rng = np.random.default_rng(4)
    jobs = mixed_jobs(rng)
    idx, dist, md, pairs = ctx.match_descriptor_jobs(jobs)
    for j, (q, t) in enumerate(jobs):
        single = ctx.match_descriptors(q, t)
        check((idx[j], dist[j], int(md[j]), pairs[j]), single)
        check(single, R.match(q, t))


def test_diagnostics_variant_equals_the_product_kernel(hip_lib, diag_lib, ctx):
    """VELO_MATCH_VARIANT=0 (diagnostics build only): XOR + popcount over u64, train rows in LDS -- bit for bit the MFMA result"""
    rng = np.random.default_rng(5)
    jobs = mixed_jobs(rng, 24) + [(rand_rows(rng, 3001), rand_rows(rng, 2999))]
    os.environ["VELO_MATCH_VARIANT"] = "0"
    try:
        dctx = api.Context(0, lib=diag_lib)
    finally:
        del os.environ["VELO_MATCH_VARIANT"]
    try:
        a = dctx.match_descriptor_jobs(jobs)
    finally:
        dctx.close()
    b = ctx.match_descriptor_jobs(jobs)
    for j in range(len(jobs)):
        check((a[0][j], a[1][j], int(a[2][j]), a[3][j]), (b[0][j], b[1][j], int(b[2][j]), b[3][j]))


def test_match_between_registrations_changes_nothing(hip_lib):
    """a 64-job match call on a context between (and inside) registrations: the same poses and counts as a context that never matched"""
    d = synth.scan_pair(n_beams=16, n_azimuth=128)
    jobs = mixed_jobs(np.random.default_rng(6))

    def counts(s):
        return (s.n_solves, s.n_assoc_rounds, s.n_queries, s.n_target,
                [(s.solves[i].lm_iterations, s.solves[i].termination) for i in range(s.n_solves)])

    plain = api.Context(0, icp_skip=1)
    mixed = api.Context(0, icp_skip=1)
    try:
        plain.set_target(d["tgt_xyz"], d["tgt_off"])
        plain.set_source(d["src_xyz"], d["src_off"])
        xa, Ta, sa = plain.frame_to_frame(d["x0"])
        mixed.match_descriptor_jobs(jobs)
        mixed.set_target(d["tgt_xyz"], d["tgt_off"])
        mixed.match_descriptor_jobs(jobs)                      # between loading the scans and registering them
        mixed.set_source(d["src_xyz"], d["src_off"])
        xb, Tb, sb = mixed.frame_to_frame(d["x0"])
        mixed.match_descriptor_jobs(jobs)
        xc, Tc, sc = mixed.frame_to_frame(d["x0"])             # the same scans again, after another match call
        xd, Td, sd = plain.frame_to_frame(d["x0"])
    finally:
        plain.close()
        mixed.close()
    assert np.array_equal(xa, xb) and np.array_equal(Ta, Tb) and counts(sa) == counts(sb)
    assert np.array_equal(xc, xd) and np.array_equal(Tc, Td) and counts(sc) == counts(sd)


def test_cxx_adaptor_matches_the_restatement(tmp_path, hip_lib):
    exe = compile_driver(tmp_path)
    rng = np.random.default_rng(7)
    n_frames = 5
    desc = [[rand_rows(rng, int(rng.integers(0 if fr == 3 else 1, 900))) for fr in range(n_frames)] for _ in range(2)]
    desc[1][2], _ = near_duplicates(rng, desc[1][0], rng.integers(0, 13, min(len(desc[1][0]), 400)))
    strides = [[64 if (c + fr) % 2 else 80 for fr in range(n_frames)] for c in range(2)]    # every other matrix a ROI-like stride
    ids = [[[] for _ in range(n_frames)] for _ in range(2)]
    case = str(tmp_path / "case.bin")
    write_case(case, desc, ids, strides)
    out = subprocess.run([exe, case, "match"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    rows = [r for r in parse(out.stdout) if r[0].startswith("mf_")]
    want = [R.match(desc[0][0], desc[1][1])[3]]                                   # matchFeatures(descriptors, 0, 1, 0, 1, m)
    want += [R.match(desc[c][0], desc[c][2])[3] for c in range(2)]                # matchFeatures(descriptors, 0, 2, m)
    want += [R.match(desc[c][0], desc[c][fr])[3] for fr in range(1, n_frames) for c in range(2)]   # matchFeaturesBatch(descriptors, 0, {1..4}, m)
    assert [r[0] for r in rows] == ["mf_cam01"] + ["mf_frame"] * 2 + ["mf_batch"] * (2 * (n_frames - 1))
    for (name, got), w in zip(rows, want):
        assert np.array_equal(got, w), name
