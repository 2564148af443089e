"""velo_graph_edge_gate and velo_graph_loop_candidates against tests/pose_graph_gate_ref.py.  The restatement is evaluated at the bytes
graph_get_poses returns, once at the loaded state and once after graph_optimize(linear_solver="envelope"), so nothing here depends on
solver parity.  What each graph is for:

  free1            a pair with a fixed end; both ends fixed      free2, chain5, large_rotation   small, large rotations
  chain12_tree     Sigma_rel across an edge is W_e^-1            chain250_split                  a pair across two components
  hub140           a row of 128 blocks, long columns
  ring70_open      held-back edges with their information: the gate itself; pairs outside the envelope chosen with api.graph_order;
                   several pairs that share a `to` frame whose column sits at position 0, at n - 1 and in the middle of the order
  lap454_open      the candidates of two queries after the solve, 462 held loop measurements through the gate
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pose_graph_cov_ref as R
import pose_graph_gate_ref as Q
import pose_graph_ref as G
import velo_amd  # noqa: F401
from test_gpu_pose_graph_covariance import load, poses_of, state_bytes, summary_bytes
from test_pose_graph_gate_cpu import MOVED, SPREAD_REL, TREE
from velo_amd import api

pytestmark = pytest.mark.gpu

# SPREAD_REL: what the restatement's own two routes to Sigma differ by (tests/test_pose_graph_gate_cpu.py).  The kernels may differ from
# the restatement by 100 x that, the project's margin for the summation order and the compiler's contraction.  The units:
#   S      sigma_i sigma_j, the square roots of the restatement's diagonal (as SPREAD_REL is measured)
#   rel, r the larger of 1 and the largest coordinate of the two poses: the translations are differences of such coordinates
#   chi2   relative to the restatement's chi2 where a record of chi2 exists: the held edges of the two open graphs, "<graph>/chi2".  On the
#          eight graphs of check() there is no such record (their pairs carry no information and many an r of rounding size, whose chi2
#          has no digits), so there chi2 is NOT compared with the restatement's: r and S are, and chi2 must be r^T S^-1 r of the RETURNED
#          r and S to 100 eps cond(S), the bound of a backward-stable solve.  That is another bound than the 100 x SPREAD_REL of r and S.
TOL = {k: 100.0 * v for k, v in SPREAD_REL.items()}
EPS = np.finfo(np.float64).eps
GRAPHS = ("free1", "free2", "chain5", "large_rotation", "chain12_tree", "chain250_split", "hub140", "ring70_open")


def library_order(g, prob):
    ea, eb = R.free_edges(g, prob)
    perm, first, stats = api.graph_order(prob.n_free, ea, eb)
    pos = np.empty(prob.n_free, dtype=np.int64)
    pos[np.asarray(perm, dtype=np.int64)] = np.arange(prob.n_free)
    return np.asarray(perm), np.asarray(first), pos, stats


@functools.lru_cache(maxsize=None)
def case(name):
    """the graph, its problem and the request (from, to, z); for ring70_open also the pairs that share a column"""
    g, prob = Q.fixture(name)
    perm, first, pos, stats = library_order(g, prob)
    outside = [(prob.free[a], prob.free[b]) for a, b in R.outside_pairs(perm, first)]
    is_out = lambda a, b: first[max(pos[prob.slot[a]], pos[prob.slot[b]])] > min(pos[prob.slot[a]], pos[prob.slot[b]])   # noqa: E731
    assert all(is_out(a, b) for a, b in outside)                       # chosen with the library's order, and outside its envelope
    shared = []
    if name == "ring70_open":                                          # three pairs each into the column at position 0, n - 1, the middle
        n = prob.n_free
        for q in (0, n - 1, n // 2):
            tq = prob.free[int(perm[q])]
            others = [prob.free[int(perm[o])] for o in range(n) if o != q and is_out(prob.free[int(perm[o])], tq)]
            assert len(others) >= 3
            shared += [(others[0], tq), (others[len(others) // 2], tq), (others[-1], tq)]
        outside = outside + shared
    if name == "chain250_split":
        assert stats["components"] == 2 and is_out(100, 200)
    frm, to, z, _ = Q.tested_pairs(name, g, prob, outside)
    return g, prob, np.asarray(frm, np.int32), np.asarray(to, np.int32), z, outside


def sigma_at(g, prob, poses):
    at = Q.at_poses(g, prob, poses)
    return at, R.by_inverse(R.dense_jacobian(at))


def compare(name, label, got, want, poses, frm, to, fixed, chi2_key=None):
    """the worst differences of (rel, r, S, chi2), each in its unit"""
    worst = dict(rel=0.0, r=0.0, S=0.0, chi2=0.0, solve=0.0)
    for p, (a, b) in enumerate(zip(frm.tolist(), to.tolist())):
        scale = max(1.0, float(np.max(np.abs(poses[a]))), float(np.max(np.abs(poses[b]))))
        worst["rel"] = max(worst["rel"], float(np.max(np.abs(got[0][p] - want[0][p]))) / scale)
        worst["r"] = max(worst["r"], float(np.max(np.abs(got[1][p] - want[1][p]))) / scale)
        Sg, Sw = got[2][p], want[2][p]
        assert Sg.tobytes() == np.ascontiguousarray(Sg.T).tobytes(), (a, b)              # symmetric to the bit
        if a in fixed and b in fixed and chi2_key is None:
            assert np.all(Sg == 0.0) and got[3][p] == -1.0, (a, b)                       # no uncertainty at all: not positive definite
            continue
        worst["S"] = max(worst["S"], Q.rel_spread(Sw, Sg))
        assert got[3][p] >= 0.0, (a, b)
        mine = float(got[1][p] @ np.linalg.solve(Sg, got[1][p]))                          # r^T S^-1 r of what was returned
        bound = 100.0 * EPS * np.linalg.cond(Sg)
        worst["solve"] = max(worst["solve"], abs(got[3][p] - mine) / max(mine, 1e-300) / bound if mine > 0.0 else 0.0)
        if chi2_key:
            worst["chi2"] = max(worst["chi2"], abs(got[3][p] - want[3][p]) / want[3][p])
    print(f"{name} ({label}): {len(frm)} pairs: rel {worst['rel']:.2e}, r {worst['r']:.2e}, S {worst['S']:.2e} sigma_i sigma_j (tolerance {TOL[name]:.2e}); "
          f"chi2 {worst['chi2']:.2e} relative; chi2 against r^T S^-1 r of the returned r, S: {worst['solve']:.2e} of 100 eps cond(S)")
    assert worst["rel"] <= TOL[name] and worst["r"] <= TOL[name] and worst["S"] <= TOL[name]
    assert worst["solve"] <= 1.0
    if chi2_key:
        assert worst["chi2"] <= TOL[chi2_key]
    return worst


def check(name, ctx, label):
    g, prob, frm, to, z, outside = case(name)
    poses = poses_of(ctx, g)
    at, S = sigma_at(g, prob, poses)
    want = Q.gate(S, at, poses, frm, to, z)
    got = ctx.graph_edge_gate(frm, to, z, None, g["fixed"])
    again = ctx.graph_edge_gate(frm, to, z, None, g["fixed"])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))                   # two identical calls, identical bytes
    assert got[0].shape == (len(frm), 6) and got[2].shape == (len(frm), 6, 6)
    compare(name, label, got, want, poses, frm, to, g["fixed"])
    # without a measurement the residual is zero to rounding, on EVERY pair: the issue's bound, whatever the distance of the two frames
    rel0, r0, cov0, _ = ctx.graph_edge_gate(frm, to, None, None, g["fixed"])
    assert rel0.tobytes() == got[0].tobytes()
    norms = np.linalg.norm(r0, axis=1)
    k = int(np.argmax(norms))
    apart = float(np.linalg.norm(poses[int(frm[k])][3:] - poses[int(to[k])][3:]))
    print(f"{name} ({label}): z = None: |r| at most {norms.max():.2e} over all {len(frm)} pairs, at ({frm[k]}, {to[k]}), {apart:.1f} m apart")
    assert norms.max() <= 1e-14
    rel1, cov1 = ctx.graph_relative_covariance(np.stack([frm, to], axis=1), g["fixed"])
    assert rel1.tobytes() == rel0.tobytes() and cov1.tobytes() == cov0.tobytes()
    return got, poses, S, at


@pytest.mark.parametrize("name", GRAPHS)
def test_gate_equals_the_restatement_before_and_after_a_solve(name):
    g, prob, frm, to, z, outside = case(name)
    ctx = api.Context(0)
    load(ctx, g)
    kept = state_bytes(ctx, g)
    got, poses, S, at = check(name, ctx, "loaded")
    assert state_bytes(ctx, g) == kept and ctx.graph_info()["optimizations"] == 0
    if name == "chain12_tree":                                         # the tree property, against numbers that are exact
        worst = max(Q.rel_spread(np.linalg.inv(e[3]), c) for e, c in zip(g["edges"], got[2]))
        print(f"chain12_tree: Sigma_rel across an edge against W_e^-1: {worst:.2e} (tolerance {100 * TREE:.1e})")
        assert worst <= 100 * TREE
    if name == "chain250_split":                                       # across the components only the two marginals count
        p = [k for k, (a, b) in enumerate(zip(frm.tolist(), to.tolist())) if (a, b) == (100, 200)][0]
        _, _, _, A, B = Q.pair_terms(poses, 100, 200, z[p])
        alone = A @ Q.block(S, at, 100, 100) @ A.T + B @ Q.block(S, at, 200, 200) @ B.T
        assert Q.rel_spread(alone, got[2][p]) <= TOL[name]
    if name in ("hub140", "ring70_open"):
        assert len(outside) >= 3
    s = ctx.graph_optimize(g["fixed"], linear_solver="envelope")
    assert s.n_free == prob.n_free
    check(name, ctx, "optimised")
    ctx.close()


def test_the_gate_separates_the_held_edges_of_ring70_open():
    g, prob, *_ = case("ring70_open")
    ctx = api.Context(0)
    load(ctx, g)
    frm, to = np.array([e[0] for e in g["held"]], np.int32), np.array([e[1] for e in g["held"]], np.int32)
    z, info = np.array([e[2] for e in g["held"]]), np.array([e[3] for e in g["held"]])
    true = np.array([k in g["true_held"] for k in range(len(frm))])
    start = ctx.graph_edge_gate(frm, to, z, info, g["fixed"])[3]
    ctx.graph_optimize(g["fixed"], linear_solver="envelope")
    poses = poses_of(ctx, g)
    at, S = sigma_at(g, prob, poses)
    got = ctx.graph_edge_gate(frm, to, z, info, g["fixed"])
    packed = ctx.graph_edge_gate(frm, to, z, np.array([Q.W.info21(w) for w in info]), g["fixed"])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, packed))                  # the two forms of info
    compare("ring70_open", "held, optimised", got, Q.gate(S, at, poses, frm, to, z, info), poses, frm, to, g["fixed"], "ring70_open/chi2")
    print("ring70_open: chi2 of the held edges " + ", ".join(f"({a}, {b}) {c:.1f}" for a, b, c in zip(frm, to, got[3])) + f"; the true edge before optimising {start[true][0]:.1f}")
    assert true.sum() == 1 and np.all(got[3][true] < 30.0) and np.all(got[3][~true] > 300.0) and len(frm) == 4
    ctx.close()


def raw_candidates(ctx, fixed, query, min_gap, radius, k_sigma, capacity):
    fx = np.asarray(fixed, dtype=np.int32)
    frames, dist, sigma = np.full(max(capacity, 1), -7, np.int32), np.full(max(capacity, 1), 7.0), np.full(max(capacity, 1), 7.0)
    found = C.c_int32(-7)
    vp = lambda v: C.c_void_p(v.ctypes.data)                          # noqa: E731
    st = ctx._lib.velo_graph_loop_candidates(ctx._h, vp(fx), len(fx), None, query, min_gap, radius, k_sigma, capacity, vp(frames), vp(dist), vp(sigma), C.byref(found))
    msg = ctx._lib.velo_last_error()
    return st, (msg.decode() if msg else ""), frames, dist, sigma, found.value


def test_candidates_and_the_gate_on_lap454_open_after_the_solve():
    g, prob = Q.fixture("lap454_open")
    ctx = api.Context(0)
    load(ctx, g)
    ctx.graph_optimize(g["fixed"], linear_solver="envelope")
    poses = poses_of(ctx, g)
    at, S = sigma_at(g, prob, poses)
    tol = TOL["lap454_open"]
    for query in (320, 453, 0):                                        # 0 is the fixed frame: no column
        lists = {}
        for radius, k in ((3.0, 0.0), (3.0, 3.0), (1.0, 2.0)):
            frames, dist, sigma, margin = Q.candidates(S, at, poses, query, 50, radius, k)
            assert margin.min() > 1e-6, (query, radius, k, margin.min())      # no frame close enough to its threshold to change sides
            want = dist <= radius + k * sigma
            gf, gd, gs = ctx.graph_loop_candidates(query, 50, radius, k, g["fixed"])
            lists[(radius, k)] = gf.tolist()
            assert gf.tolist() == frames[want].tolist(), (query, radius, k)
            assert np.max(np.abs(gd - dist[want])) <= tol * max(1.0, float(np.max(np.abs(poses[query]))))
            if k > 0.0:
                assert np.max(np.abs(gs - sigma[want]) / sigma[want]) <= tol
            else:
                assert np.all(gs == 0.0)
            print(f"lap454_open, query {query}, radius {radius}, k_sigma {k}: {len(gf)} candidates {gf.tolist()}, closest margin {margin.min():.1e}")
        assert set(lists[(3.0, 0.0)]) <= set(lists[(3.0, 3.0)]) and len(lists[(3.0, 3.0)]) > len(lists[(3.0, 0.0)]) or query == 0
        full = lists[(3.0, 3.0)]
        if len(full) > 2:                                              # a capacity of 2: the first two, the count unchanged
            st, _, f2, d2, s2, found = raw_candidates(ctx, g["fixed"], query, 50, 3.0, 3.0, 2)
            assert st == 0 and found == len(full) and f2.tolist() == full[:2]
            small = ctx.graph_loop_candidates(query, 50, 3.0, 3.0, g["fixed"], capacity=2)
            assert small[0].tolist() == full                           # the Python entry asks again
    # the 462 held loop measurements through the gate, and moved 3 m off
    frm, to = np.array([e[0] for e in g["held"]], np.int32), np.array([e[1] for e in g["held"]], np.int32)
    z, info = np.array([e[2] for e in g["held"]]), np.array([e[3] for e in g["held"]])
    got = ctx.graph_edge_gate(frm, to, z, info, g["fixed"])
    compare("lap454_open", "held, optimised", got, Q.gate(S, at, poses, frm, to, z, info), poses, frm, to, g["fixed"], "lap454_open/chi2")
    off = ctx.graph_edge_gate(frm, to, z + MOVED, info, g["fixed"])[3]
    print(f"lap454_open: chi2 of {len(frm)} held loop measurements: median {np.median(got[3]):.1f}, max {got[3].max():.1f}; moved 3 m off: min {off.min():.1f}")
    assert got[3].max() < 30.0 and off.min() > 300.0
    ctx.close()


def test_distances_alone_serve_a_graph_whose_h_is_singular():
    g = G.fixture("hub")                                               # as shipped: frame 140 is free and no edge touches it
    ctx = api.Context(0)
    load(ctx, g)
    kept = state_bytes(ctx, g)
    for query, radius in ((1, 6.0), (0, 5.0), (140, 12.0)):            # a fixed frame, the hub, the frame without edges (10 to 18 m from the rim)
        gf, gd, gs = ctx.graph_loop_candidates(query, 3, radius, 0.0, g["fixed"])
        frames = np.array([f for f in sorted(g["poses"]) if abs(f - query) >= 3])
        dist = np.array([np.linalg.norm(Q.relative(g["poses"][f], g["poses"][query])[3:]) for f in frames])
        assert gf.tolist() == frames[dist <= radius].tolist() and 0 < len(gf) < len(frames), query
        assert np.max(np.abs(gd - dist[dist <= radius])) <= 100 * EPS * 10.0 and np.all(gs == 0.0)
    with pytest.raises(api.VeloError, match="status -1.*velo_graph_loop_candidates.*not positive definite.*frame 140"):
        ctx.graph_loop_candidates(0, 3, 6.0, 1.0, g["fixed"])
    assert state_bytes(ctx, g) == kept and ctx.graph_info()["optimizations"] == 0
    ctx.close()


@pytest.mark.parametrize("name", ["ring70_open"])
def test_asking_changes_nothing_a_solve_sees(name):
    g, prob, frm, to, z, _ = case(name)
    asked, plain = api.Context(0), api.Context(0)
    load(asked, g)
    load(plain, g)
    ask = lambda: (asked.graph_edge_gate(frm, to, z, None, g["fixed"]), asked.graph_loop_candidates(40, 5, 3.0, 3.0, g["fixed"]),   # noqa: E731
                   asked.graph_loop_candidates(40, 5, 3.0, 0.0, g["fixed"]))
    ask()
    assert state_bytes(asked, g) == state_bytes(plain, g)
    assert asked.graph_info() == plain.graph_info() and asked.graph_info()["optimizations"] == 0
    pairs = np.stack([frm, to], axis=1)[:40]
    out = []
    for ctx in (asked, plain):
        for solver in ("envelope", "cg"):
            s = ctx.graph_optimize(g["fixed"], linear_solver=solver)
            out.append(summary_bytes(s) + state_bytes(ctx, g))
            if ctx is asked:
                ask()
            out.append(ctx.graph_covariance(pairs, g["fixed"]).tobytes())
    assert out[:4] == out[4:]
    assert asked.graph_info() == plain.graph_info()
    asked.close()
    plain.close()


def raw_gate(ctx, fixed, frm, to, z=None, info=None, max_work=None):
    """the C-ABI itself, with outputs the test owns: (status, message, the outputs)"""
    fx = np.asarray(fixed, dtype=np.int32)
    a, b = np.asarray(frm, dtype=np.int32), np.asarray(to, dtype=np.int32)
    outs = [np.full((len(a), k), 7.0) for k in (6, 6, 36, 1)]
    p = api.VeloGraphParams()
    p.cg_tolerance, p.cg_max_iterations = 1e-10, 2000
    p.reserved[1] = 0 if max_work is None else max_work
    vp = lambda v: None if v is None else C.c_void_p(np.ascontiguousarray(v, dtype=np.float64).ctypes.data)   # noqa: E731
    zz = None if z is None else np.ascontiguousarray(z, dtype=np.float64)
    ww = None if info is None else np.ascontiguousarray(info, dtype=np.float64)
    st = ctx._lib.velo_graph_edge_gate(ctx._h, C.c_void_p(fx.ctypes.data), len(fx), C.byref(p), len(a), C.c_void_p(a.ctypes.data), C.c_void_p(b.ctypes.data),
                                       None if zz is None else C.c_void_p(zz.ctypes.data), None if ww is None else C.c_void_p(ww.ctypes.data),
                                       *[C.c_void_p(o.ctypes.data) for o in outs])
    msg = ctx._lib.velo_last_error()
    return st, (msg.decode() if msg else ""), outs


def test_refusals_leave_the_outputs_and_the_store_alone():
    g = G.fixture("hub")                                               # as shipped: frame 140 is free and no edge touches it
    ctx = api.Context(0)
    load(ctx, g)
    kept = state_bytes(ctx, g)
    untouched = lambda outs: all(np.all(o == 7.0) for o in outs)      # noqa: E731
    st, msg, outs = raw_gate(ctx, g["fixed"], [0, 5], [5, 9])
    assert st == -1 and "velo_graph_edge_gate" in msg and "not positive definite" in msg and "frame 140" in msg and untouched(outs)
    fixed = [1, 2, 140]
    st, msg, outs = raw_gate(ctx, fixed, [0, 5, 1], [5, 9, 2])         # with 140 fixed as well the same store answers
    assert st == 0 and np.all(np.diag(outs[2][0].reshape(6, 6)) > 0.0) and outs[3][2, 0] == -1.0 and np.all(outs[2][2] == 0.0)
    _, prob = R.fixture("hub140")
    ea, eb = R.free_edges(dict(edges=g["edges"]), prob)
    _, _, stats = api.graph_order(prob.n_free, ea, eb)
    st, msg, outs = raw_gate(ctx, fixed, [0], [5], max_work=stats["work"] - 1)
    assert st == -1 and f"velo_graph_edge_gate: the envelope solver's work is {stats['work']} block products, over the cap of {stats['work'] - 1} " in msg and untouched(outs)
    assert raw_gate(ctx, fixed, [0], [5], max_work=stats["work"])[0] == 0
    W = np.eye(6)
    bad_w = Q.W.info21(np.diag([1.0, 1.0, -1.0, 1.0, 1.0, 1.0]))
    nan_z = np.zeros((2, 6))
    nan_z[1, 4] = np.nan
    for frm, to, z, info, status, text in (([0], [141], None, None, -3, "pair 0 names frame 141, which has no pose"),
                                           ([0, -1], [5, 0], None, None, -1, "pair 1: frames -1 -> 0"),
                                           ([0], [1 << 22], None, None, -1, "pair 0: frames"),
                                           ([0, 7], [5, 7], None, None, -1, "pair 1: from == to (7)"),
                                           ([0, 7], [5, 8], nan_z, None, -1, "pair 1: z[4] is not finite"),
                                           ([0, 7], [5, 8], None, [Q.W.info21(W), bad_w], -1, "pair 1: its information matrix is not positive definite"),
                                           ([0], [5], None, [np.full(21, np.inf)], -1, "pair 0: info21[0] is not finite")):
        st, msg, outs = raw_gate(ctx, fixed, frm, to, z, info)
        assert st == status and text in msg and untouched(outs), (frm, to, st, msg)
    one = np.zeros(1, dtype=np.int32)
    fx = np.asarray(fixed, dtype=np.int32)
    vp = lambda v: C.c_void_p(v.ctypes.data)                          # noqa: E731
    nul = [None] * 6
    assert ctx._lib.velo_graph_edge_gate(ctx._h, vp(fx), 3, None, -1, vp(one), vp(one), *nul) == -1
    assert ctx._lib.velo_graph_edge_gate(ctx._h, vp(fx), 3, None, 1, None, vp(one), *nul) == -1
    assert ctx._lib.velo_graph_edge_gate(ctx._h, vp(fx), 3, None, 0, None, None, *nul) == 0
    five = np.asarray([5], dtype=np.int32)
    assert ctx._lib.velo_graph_edge_gate(ctx._h, vp(fx), 3, None, 1, vp(one), vp(five), *nul) == 0          # every output may be NULL
    with pytest.raises(api.VeloError, match="status -1.*ascending"):
        ctx.graph_edge_gate([0], [5], fixed=[2, 1])
    # the candidates' arguments
    for args, status, text in (((141, 3, 1.0, 1.0, 4), -3, "query frame 141 has no pose"), ((-1, 3, 1.0, 1.0, 4), -1, "frame"), ((0, 0, 1.0, 1.0, 4), -1, "min_gap 0"),
                               ((0, 3, -1.0, 1.0, 4), -1, "radius"), ((0, 3, 1.0, float("nan"), 4), -1, "k_sigma"), ((0, 3, 1.0, 1.0, -1), -1, "negative capacity"),
                               ((0, 3, 6.0, 1.0, 4), -1, "frame 140")):
        st, msg, frames, dist, sigma, found = raw_candidates(ctx, g["fixed"], *args)
        assert st == status and text in msg, (args, st, msg)
        assert np.all(frames == -7) and np.all(dist == 7.0) and np.all(sigma == 7.0) and found == -7
    with pytest.raises(api.VeloError, match="status -1.*velo_graph_loop_candidates: the envelope solver's work is .* over the cap of 1 "):
        ctx.graph_loop_candidates(0, 3, 6.0, 1.0, fixed, max_work=1)
    assert len(ctx.graph_loop_candidates(0, 3, 6.0, 1.0, fixed, max_work=stats["work"])[0]) > 0
    assert state_bytes(ctx, g) == kept and ctx.graph_info()["optimizations"] == 0
    ctx.close()
