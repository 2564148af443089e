"""velo_graph_order, the order the envelope solver of velo_graph_optimize factors in, against tests/graph_order_ref.py (the rule of
include/velo_hip.h restated in pure Python): no GPU.  Also what the envelope solver's GPU test rests on and can be checked here: the
header's constants and the refusals, the bookkeeping of a permuted solve, and -- on the graphs of tests/pose_graph_env_fixtures.py --
that the restatement's two linear solvers take the same LM decisions, with the spread between them that
tests/test_gpu_pose_graph_envelope.py derives its tolerances from."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla
from scipy.sparse.csgraph import reverse_cuthill_mckee

import graph_order_ref as R
import pose_graph_env_fixtures as F
import pose_graph_ref as G
import velo_amd  # noqa: F401
from velo_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build_hip()
    return api.load_library()


def lap():
    odometry, loops = F.lap_edges()
    return F.LAP_N, [e[0] for e in odometry + loops], [e[1] for e in odometry + loops]


def star(n=131, hub=17):
    leaves = [v for v in range(n) if v != hub]
    return n, [hub if k % 2 else v for k, v in enumerate(leaves)], [v if k % 2 else hub for k, v in enumerate(leaves)]


def graphs():
    path = [3, 0, 4, 1, 2]                                             # a path of 5 in shuffled numbering
    two = ([0, 2, 4, 6, 1, 3, 5], [2, 4, 6, 8, 3, 5, 1])               # the path 0-2-4-6-8, the triangle 1-3-5, node 7 alone
    return {
        "single": (1, [], []),
        "pair": (2, [0], [1]),
        "path5": (5, path[:-1], path[1:]),
        "ring70": (70, [i for d in (1, 2, 3, 4) for i in range(70)], [(i + d) % 70 for d in (1, 2, 3, 4) for i in range(70)]),
        "star131": star(),
        "two_components_and_a_loner": (9, two[0], two[1]),
        "duplicates": (4, [0, 1, 0, 1, 2, 3, 2], [1, 0, 1, 2, 1, 2, 3]),
        "lap454": lap(),
    }


GRAPHS = graphs()


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_order_equals_the_restatement(name):
    n, a, b = GRAPHS[name]
    perm, first, stats = api.graph_order(n, a, b)
    want_perm, want_first, want_stats = R.order(n, a, b)
    assert perm.tolist() == want_perm.tolist()
    assert first.tolist() == want_first.tolist()
    assert (stats["widest_row"], stats["envelope_blocks"], stats["work"], stats["components"]) == want_stats
    # a permutation; first and the statistics follow from it by definition
    assert sorted(perm.tolist()) == list(range(n))
    pos = {int(v): k for k, v in enumerate(perm)}
    nb = [set() for _ in range(n)]
    for u, v in zip(a, b):
        nb[u].add(v)
        nb[v].add(u)
    by_definition = [min([k] + [pos[v] for v in nb[int(perm[k])]]) for k in range(n)]
    assert first.tolist() == by_definition
    w = [k - f for k, f in enumerate(by_definition)]
    assert (stats["widest_row"], stats["envelope_blocks"], stats["work"]) == (max(w), sum(x + 1 for x in w), sum(x * (x + 1) // 2 for x in w))


def test_named_properties_of_the_orders():
    perm, first, stats = api.graph_order(*GRAPHS["single"])
    assert (perm.tolist(), first.tolist(), stats) == ([0], [0], dict(widest_row=0, envelope_blocks=1, work=0, components=1))
    _, _, stats = api.graph_order(*GRAPHS["pair"])
    assert stats == dict(widest_row=1, envelope_blocks=3, work=1, components=1)
    perm, _, stats = api.graph_order(*GRAPHS["path5"])                # a path is walked from one end to the other: band width 1
    assert perm.tolist() in ([3, 0, 4, 1, 2], [2, 1, 4, 0, 3]) and stats["widest_row"] == 1 and stats["envelope_blocks"] == 9
    n, a, b = GRAPHS["star131"]
    perm, _, stats = api.graph_order(n, a, b)                          # the hub neither first nor last: a leaf on either side of it
    assert perm[0] != 17 and stats["envelope_blocks"] <= 2 * 131 and stats["components"] == 1
    perm, first, stats = api.graph_order(*GRAPHS["two_components_and_a_loner"])
    assert stats["components"] == 3
    # the sequence of the components is reversed as a whole: the loner (7) before the component of 1, that before the component of 0
    where = {int(v): k for k, v in enumerate(perm)}
    assert max(where[v] for v in (7,)) < min(where[v] for v in (1, 3, 5)) and max(where[v] for v in (1, 3, 5)) < min(where[v] for v in (0, 2, 4, 6, 8))
    assert first[where[7]] == where[7]                                # a row of width 0
    # duplicate and reversed edges are merged: the order of the path 0-1-2-3 given once
    once = api.graph_order(4, [0, 1, 2], [1, 2, 3])
    many = api.graph_order(*GRAPHS["duplicates"])
    assert once[0].tolist() == many[0].tolist() and once[1].tolist() == many[1].tolist() and once[2] == many[2]


def test_lap_graph_is_no_wider_than_one_and_a_half_of_scipys():
    n, a, b = GRAPHS["lap454"]
    _, _, stats = api.graph_order(n, a, b)
    M = sp.coo_matrix((np.ones(len(a)), (a, b)), shape=(n, n))
    theirs = reverse_cuthill_mckee((M + M.T).tocsr(), symmetric_mode=True)
    _, (widest, blocks, work) = R.stats_of(R.neighbours(n, a, b), theirs)
    print(f"lap454: widest row / envelope blocks / work: velo_graph_order {stats['widest_row']} / {stats['envelope_blocks']} / {stats['work']}, "
          f"scipy reverse_cuthill_mckee {widest} / {blocks} / {work}")
    assert stats["widest_row"] <= 1.5 * widest
    assert stats["envelope_blocks"] <= 1.5 * blocks


def test_refusals(lib):
    n = 3
    a, b = (C.c_int32 * 2)(0, 1), (C.c_int32 * 2)(1, 2)
    perm, first, stats = (C.c_int32 * n)(), (C.c_int32 * n)(), (C.c_int64 * 4)()
    assert lib.velo_graph_order(n, 2, a, b, perm, first, stats) == 0 and sorted(perm) == [0, 1, 2]
    for args in ((n, 2, None, b, perm, first, stats), (n, 2, a, None, perm, first, stats), (n, 2, a, b, None, first, stats),
                 (n, 2, a, b, perm, None, stats), (n, 2, a, b, perm, first, None), (-1, 0, None, None, perm, first, stats), (n, -1, a, b, perm, first, stats)):
        assert lib.velo_graph_order(*args) == -1
    assert lib.velo_graph_order(n, 0, None, None, perm, first, stats) == 0 and stats[3] == 3      # no edge: three components
    for bad in ((0, 3), (-1, 1), (1, 1)):                              # an end out of range, a == b
        ba, bb = (C.c_int32 * 2)(0, bad[0]), (C.c_int32 * 2)(1, bad[1])
        assert lib.velo_graph_order(n, 2, ba, bb, perm, first, stats) == -1
    assert b"a == b" in lib.velo_last_error()
    # velo_graph_optimize still refuses a null context before it looks at anything else, the solver included
    p = api.VeloGraphParams()
    assert lib.velo_default_graph_params(C.byref(p)) == 0 and list(p.reserved) == [0] * 5
    p.reserved[0] = 7
    fixed = (C.c_int32 * 1)(0)
    assert lib.velo_graph_optimize(None, fixed, 1, C.byref(p), None) == -1 and b"null ctx" in lib.velo_last_error()


PROBE = r'''
#include <stdio.h>
#include <stddef.h>
#include "velo_hip.h"
int main(void) {
  velo_graph_params p;
  printf("%zu %zu %zu %d %d %d\n", sizeof(velo_graph_params), offsetof(velo_graph_params, reserved), sizeof(p.reserved) / sizeof(p.reserved[0]),
         VELO_GRAPH_SOLVER_CG, VELO_GRAPH_SOLVER_ENVELOPE, VELO_GRAPH_DEFAULT_MAX_WORK);
  return 0; }
'''


def test_header_constants_and_struct_size(tmp_path):
    cfile, exe = str(tmp_path / "probe.c"), str(tmp_path / "probe")
    open(cfile, "w").write(PROBE)
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe], check=True)
    row = [int(v) for v in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.split()]
    assert row == [32, api.VeloGraphParams.reserved.offset, 5, api.GRAPH_SOLVER_CG, api.GRAPH_SOLVER_ENVELOPE, api.GRAPH_DEFAULT_MAX_WORK] == [32, 12, 5, 0, 1, 1 << 24]
    assert C.sizeof(api.VeloGraphParams) == 32


def test_a_solve_permuted_by_the_order_is_the_solve():
    """The bookkeeping the GPU test relies on: the damped system of ring70's first LM iteration, its blocks permuted by
    velo_graph_order's perm, solved and permuted back, is the unpermuted solve to rounding."""
    g = G.fixture("ring70")
    prob = G.problem_of(g)
    _, r, J = prob.evaluate(prob.x0())
    c = 1.0 / (1.0 + np.sqrt(np.asarray(J.multiply(J).sum(axis=0)).ravel()))
    Js = J @ sp.diags(c)
    H = (Js.T @ Js).tocsr()
    d = np.clip(H.diagonal(), G.LM_DEFAULTS["d_lo"], G.LM_DEFAULTS["d_hi"])
    A, b = (H + sp.diags(d / G.LM_DEFAULTS["radius0"])).tocsc(), -(Js.T @ r)
    n, ea, eb = F.free_graph(g)
    perm, first, stats = api.graph_order(n, ea, eb)
    idx = (6 * perm.astype(np.int64)[:, None] + np.arange(6)[None, :]).ravel()
    Ap = A[idx][:, idx].tocsc()
    # every block of the permuted matrix lies inside the envelope that `first` states
    rows, cols = Ap.nonzero()
    assert np.all(cols // 6 >= first[rows // 6].astype(np.int64))
    x = spla.spsolve(A, b)
    xp = np.empty_like(x)
    xp[idx] = spla.spsolve(Ap, b[idx])
    cond = np.linalg.cond(A.toarray())
    err = np.linalg.norm(xp - x) / np.linalg.norm(x)
    print(f"ring70: permuted against unpermuted solve {err:.2e} relative, condition number {cond:.2e}, widest row {stats['widest_row']}")
    # two backward-stable direct solves of one system differ by a small multiple of cond x DBL_EPSILON
    assert err <= 64.0 * cond * G.EPS


# ---- the restatement's two solvers on the envelope test's graphs -------------------------------------------------------------------
def step_pcg_batched(A, b, o):
    """pose_graph_ref.step_pcg -- the same iteration, stopping rule and breakdown test -- with the block-Jacobi preconditioner applied to
    all blocks at once (a batched Cholesky solve) and a sparse product: the graphs here need thousands of CG iterations per LM
    iteration, which the per-block Python loop of the original takes minutes over.  test_the_batched_cg_is_the_restatements_cg holds it
    to the original."""
    n = A.shape[0] // 6
    A = A.tocsr()
    blocks = np.stack([A[6 * i:6 * i + 6, 6 * i:6 * i + 6].toarray() for i in range(n)])
    L = np.linalg.cholesky(blocks)
    Lt = np.transpose(L, (0, 2, 1))

    def precondition(v):
        return np.linalg.solve(Lt, np.linalg.solve(L, v.reshape(n, 6, 1))).reshape(-1)
    y, r = np.zeros_like(b), b.copy()
    z = precondition(r)
    rho0 = rho = float(r @ z)
    p = np.zeros_like(b)
    rho_prev, k = 1.0, 0
    while k < o["cg_max"]:
        if rho <= o["cg_tol"] ** 2 * rho0:
            break
        p = z + ((rho / rho_prev) if k > 0 else 0.0) * p
        q = A @ p
        sigma = float(p @ q)
        if not (sigma > 0.0 and np.isfinite(sigma)):
            raise np.linalg.LinAlgError("CG broke down")
        alpha = rho / sigma
        y += alpha * p
        r -= alpha * q
        z = precondition(r)
        rho_prev, rho = rho, float(r @ z)
        k += 1
    return y, k, (np.sqrt(rho / rho0) if rho0 > 0.0 else 0.0)


def test_the_batched_cg_is_the_restatements_cg(monkeypatch):
    prob = G.problem_of(G.fixture("ring70"))
    want = G.solve(prob, "pcg")
    monkeypatch.setattr(G, "step_pcg", step_pcg_batched)
    got = G.solve(prob, "pcg")
    assert [(t["status"], t["cg_iterations"]) for t in got["trace"]] == [(t["status"], t["cg_iterations"]) for t in want["trace"]]
    sc, sx = G.spread(got, want)
    print(f"ring70: batched against per-block CG: {sc:.2e} of the initial cost, {sx:.2e} in the unknowns")
    assert sc <= 1e-14 and sx <= 1e-12                                 # below the spread direct / pcg recorded for ring70


CG_CAP = 50000                                                         # high enough that CG meets its tolerance in every LM iteration
# Measured here between `direct` and `pcg` (cost: relative to the initial cost along the trace; unknowns: absolute); the GPU test
# allows 100 x these.  free1 has one free node, so block-Jacobi CG IS the direct solve: one unit of the format instead, as for
# pose_graph_ref's `pair` -- DBL_EPSILON in cost and DBL_EPSILON x 2 (the power of two above its largest pose component, 1.1) in the unknowns.
SPREAD = {"chain250": (3.3e-13, 4.5e-11), "chain250_split": (2.9e-13, 4.4e-12), "lap454": (2.1e-11, 2.9e-9), "free1": (2.3e-16, 4.5e-16),
          "free2": (8.8e-15, 3.2e-15)}


@functools.lru_cache(maxsize=None)
def both_solves(name):
    prob = G.problem_of(F.fixture(name))
    direct = G.solve(prob, "direct")
    saved = G.step_pcg
    G.step_pcg = step_pcg_batched
    try:
        pcg = G.solve(prob, "pcg", cg_max=CG_CAP)
    finally:
        G.step_pcg = saved
    return prob, direct, pcg


@pytest.mark.parametrize("name", F.ENV_FIXTURES)
def test_the_two_solvers_agree_on_the_envelope_fixtures(name):
    prob, a, b = both_solves(name)
    assert [r["status"] for r in a["trace"]] == [r["status"] for r in b["trace"]] and len(a["trace"]) >= 2
    assert a["termination"] == b["termination"] and a["iterations"] == b["iterations"] and a["evaluations"] == b["evaluations"]
    margin = min(G.closest_margin(a["trace"]), G.closest_margin(b["trace"]))
    assert margin > 1e-6, margin                                       # no decision lies near its threshold: rounding cannot flip one
    # CG met its tolerance in every LM iteration: it never ran into the cap
    assert all(r["cg_iterations"] < CG_CAP and r["cg_residual"] <= G.CG_DEFAULTS["cg_tol"] for r in b["trace"])
    sc, sx = G.spread(a, b)
    print(f"{name}: spread {sc:.2e} of the initial cost, {sx:.2e} absolute in the unknowns; closest decision margin {margin:.2e}; statuses "
          f"{[r['status'] for r in a['trace']]}; CG iterations {[r['cg_iterations'] for r in b['trace']]}; largest |unknown| {np.abs(a['x']).max():.3g}")
    assert sc <= 3 * SPREAD[name][0] and sx <= 3 * SPREAD[name][1]      # the record is what was measured, to a factor of 3 (LAPACK builds differ)
    n, ea, eb = F.free_graph(F.fixture(name))
    assert n == prob.n_free
    _, first, stats = api.graph_order(n, ea, eb)
    if name == "chain250":                                             # what the fixture is for
        assert stats["components"] == 1 and np.any(np.diff(first) < 0) and stats["widest_row"] > 2
    if name == "chain250_split":
        assert stats["components"] == 2
    if name in ("free1", "free2"):
        assert n == int(name[-1])
