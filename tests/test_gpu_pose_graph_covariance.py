"""velo_graph_covariance against tests/pose_graph_cov_ref.py: on every graph of pose_graph_cov_ref.FIXTURES all marginals, every edge's
(a, b) and (b, a), the fixed frames and three pairs outside the envelope, once at the loaded state and once after
graph_optimize(linear_solver="envelope").  The reference is np.linalg.inv(J^T J) with J evaluated at the bytes graph_get_poses
returns, so nothing here depends on solver parity.  What each graph is for:

  free1            one free node: S_j is empty          free2, chain5, large_rotation   small, large rotations
  ring70           the wrap edge                        chain250                        `first` is not monotone
  chain250_split   two components: a pair across them is exactly zero
  lap454           a column of 26 rows                  hub140                          a row of 128 blocks: the strided loops, long column solves
  ring70_outliers, chain5_mixed   matrix information and the Cauchy corrector
"""
import ctypes as C
import functools

import numpy as np
import pytest

import pose_graph_cov_ref as R
import pose_graph_ref as G
import velo_amd  # noqa: F401
from test_pose_graph_cov_cpu import SPREAD
from velo_amd import api

pytestmark = pytest.mark.gpu

# SPREAD: the largest difference between two of the restatement's three routes (tests/test_pose_graph_cov_cpu.py), normalised by
# sigma_i sigma_j.  The kernels may differ from the restatement by 100 x that: the project's margin for the summation order and the
# compiler's contraction (tests/test_gpu_pose_graph_envelope.py).
TOL = {k: 100.0 * v for k, v in SPREAD.items()}


def load(ctx, g):
    """poses in one call, the edges in runs of one kind (a number as information: the scalar entry), cut where the fixture says"""
    ctx.graph_reset(g.get("edge_capacity", 0))
    for f in sorted(g["poses"]):
        ctx.graph_set_pose(f, g["poses"][f])
    cut = g.get("split", len(g["edges"]))
    for part in (g["edges"][:cut], g["edges"][cut:]):
        k = 0
        while k < len(part):
            scalar = np.ndim(part[k][3]) == 0
            m = k
            while m < len(part) and (np.ndim(part[m][3]) == 0) == scalar:
                m += 1
            run = part[k:m]
            if scalar:
                ctx.graph_add_edges([e[0] for e in run], [e[1] for e in run], [e[2] for e in run], [e[3] for e in run])
            else:
                ctx.graph_add_edges_weighted([e[0] for e in run], [e[1] for e in run], [e[2] for e in run], np.array([e[3] for e in run]),
                                             [e[4] for e in run])
            k = m


def poses_of(ctx, g):
    return {f: ctx.graph_get_poses(f, 1)[0] for f in sorted(g["poses"])}


def state_bytes(ctx, g):
    return b"".join(p.tobytes() for p in poses_of(ctx, g).values())


def summary_bytes(s):
    return C.string_at(C.addressof(s), C.sizeof(s))


@functools.lru_cache(maxsize=None)
def case(name):
    """the graph, its problem, the library's order of its free nodes and the request: [n, 2] frames"""
    g, prob = R.fixture(name)
    ea, eb = R.free_edges(g, prob)
    perm, first, stats = api.graph_order(prob.n_free, ea, eb)
    pos = np.empty(prob.n_free, dtype=np.int64)
    pos[np.asarray(perm, dtype=np.int64)] = np.arange(prob.n_free)
    outside = [(prob.free[a], prob.free[b]) for a, b in R.outside_pairs(perm, first)]
    for a, b in outside:                                               # chosen with the library's order, and outside its envelope
        hi, lo = max(pos[prob.slot[a]], pos[prob.slot[b]]), min(pos[prob.slot[a]], pos[prob.slot[b]])
        assert first[hi] > lo
    if name == "chain250_split":                                       # one pair across the two components
        assert stats["components"] == 2
        outside.append((100, 200))
        assert first[max(pos[prob.slot[100]], pos[prob.slot[200]])] > min(pos[prob.slot[100]], pos[prob.slot[200]])
    frames = sorted(g["poses"])
    pairs = [(f, f) for f in frames]
    pairs += [(e[0], e[1]) for e in g["edges"]] + [(e[1], e[0]) for e in g["edges"]]
    pairs += [(f, frames[-1]) for f in g["fixed"]]
    pairs += outside + [(b, a) for a, b in outside]
    return g, prob, stats, outside, np.asarray(pairs, dtype=np.int32)


def reference(g, prob, poses):
    """Sigma by the inverse with J at `poses`, and its standard deviations"""
    at = type(prob)(poses, g["edges"], g["fixed"])
    J = R.dense_jacobian(at)
    S = R.by_inverse(J)
    return S, np.sqrt(np.diag(S))


def check(name, ctx, g, prob, outside, pairs, label):
    S, sigma = reference(g, prob, poses_of(ctx, g))
    got = ctx.graph_covariance(pairs, g["fixed"])
    again = ctx.graph_covariance(pairs, g["fixed"])
    assert got.shape == (len(pairs), 6, 6) and got.tobytes() == again.tobytes()           # two identical calls, identical bytes
    worst, by_pair = 0.0, {}
    for (a, b), blk in zip(pairs.tolist(), got):
        by_pair[(a, b)] = blk
        if a in g["fixed"] or b in g["fixed"]:
            assert np.all(blk == 0.0), (a, b)                          # a constant has no uncertainty: exactly zero
            continue
        ia, ib = prob.slot[a], prob.slot[b]
        worst = max(worst, R.cov_spread(blk, R.block_of(S, ia, ib), sigma[6 * ia:6 * ia + 6], sigma[6 * ib:6 * ib + 6]))
    print(f"{name} ({label}): {len(pairs)} pairs, {len(outside)} outside the envelope, worst difference {worst:.3e} sigma_i sigma_j (tolerance {TOL[name]:.3e})")
    assert worst <= TOL[name]
    for (a, b), blk in by_pair.items():
        if a in g["fixed"] or b in g["fixed"]:
            continue
        if a == b:
            assert blk.tobytes() == np.ascontiguousarray(blk.T).tobytes(), a          # a marginal is symmetric to the bit
        else:
            assert blk.tobytes() == np.ascontiguousarray(by_pair[(b, a)].T).tobytes(), (a, b)
    m = ctx.graph_covariance([f for f in sorted(g["poses"])], g["fixed"])               # the 1-D form: the marginals
    assert all(m[k].tobytes() == by_pair[(f, f)].tobytes() for k, f in enumerate(sorted(g["poses"])))
    if name == "chain250_split":
        assert np.all(by_pair[(100, 200)] == 0.0) and np.all(by_pair[(200, 100)] == 0.0)  # across the components: exactly zero
        assert np.all(np.diag(by_pair[(100, 100)]) > 0.0)
    free = [f for f in sorted(g["poses"]) if f not in g["fixed"]]
    assert all(np.all(np.diag(by_pair[(f, f)]) > 0.0) for f in free)


@pytest.mark.parametrize("name", R.FIXTURES)
def test_covariance_equals_the_restatement_before_and_after_a_solve(name):
    g, prob, stats, outside, pairs = case(name)
    ctx = api.Context(0)
    load(ctx, g)
    kept = state_bytes(ctx, g)
    check(name, ctx, g, prob, outside, pairs, "loaded")
    assert state_bytes(ctx, g) == kept and ctx.graph_info()["optimizations"] == 0
    s = ctx.graph_optimize(g["fixed"], linear_solver="envelope")
    assert s.n_free == prob.n_free
    check(name, ctx, g, prob, outside, pairs, "optimised")
    if name in ("ring70", "lap454", "hub140", "chain250"):
        assert len(outside) == 3
    if name == "free1":
        assert prob.n_free == 1 and stats["widest_row"] == 0
    if name == "lap454":
        assert stats["widest_row"] >= 25
    if name == "hub140":
        assert stats["widest_row"] + 1 >= 128
    # the joint covariance: the three blocks of one call
    a, b = (pairs[-1] if len(outside) else pairs[len(g["poses"])]).tolist()
    if a not in g["fixed"] and b not in g["fixed"] and a != b:
        J = ctx.graph_joint_covariance(a, b, g["fixed"])
        blk = ctx.graph_covariance([[a, a], [a, b], [b, b]], g["fixed"])
        assert np.array_equal(J[:6, :6], blk[0]) and np.array_equal(J[:6, 6:], blk[1]) and np.array_equal(J[6:, 6:], blk[2]) and np.array_equal(J, J.T)
        assert np.all(np.linalg.eigvalsh(J) > 0.0)
    ctx.close()


@pytest.mark.parametrize("name", ["ring70", "ring70_outliers"])
def test_asking_for_a_covariance_changes_nothing_a_solve_sees(name):
    g, prob, _, _, pairs = case(name)
    asked, plain = api.Context(0), api.Context(0)
    load(asked, g)
    load(plain, g)
    asked.graph_covariance(pairs, g["fixed"])
    assert state_bytes(asked, g) == state_bytes(plain, g)
    assert asked.graph_info() == plain.graph_info() and asked.graph_info()["optimizations"] == 0
    out = []
    for ctx in (asked, plain):
        for solver in ("envelope", "cg"):
            s = ctx.graph_optimize(g["fixed"], linear_solver=solver)
            out.append(summary_bytes(s) + state_bytes(ctx, g))
            if ctx is asked:
                ctx.graph_covariance(pairs[:5], g["fixed"])
    assert out[0] == out[2] and out[1] == out[3]
    assert asked.graph_info() == plain.graph_info()
    asked.close()
    plain.close()


def raw_call(ctx, fixed, pairs, max_work=None):
    """the C-ABI itself, with an output the test owns: (status, message, the output)"""
    fx = np.asarray(fixed, dtype=np.int32)
    a = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32)[:, 0])
    b = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32)[:, 1])
    out = np.full((len(a), 36), 7.0)
    p = api.VeloGraphParams()
    p.cg_tolerance, p.cg_max_iterations = 1e-10, 2000
    p.reserved[1] = 0 if max_work is None else max_work
    vp = lambda v: C.c_void_p(v.ctypes.data)                          # noqa: E731
    st = ctx._lib.velo_graph_covariance(ctx._h, vp(fx), len(fx), C.byref(p), len(a), vp(a), vp(b), vp(out))
    msg = ctx._lib.velo_last_error()
    return st, (msg.decode() if msg else ""), out


def test_refusals_leave_the_output_and_the_store_alone():
    g = G.fixture("hub")                                               # as shipped: frame 140 is free and no edge touches it
    ctx = api.Context(0)
    load(ctx, g)
    kept = state_bytes(ctx, g)
    st, msg, out = raw_call(ctx, g["fixed"], [(0, 0), (5, 0)])
    assert st == -1 and "not positive definite" in msg and "frame 140" in msg and np.all(out == 7.0)
    with pytest.raises(api.VeloError, match="status -1.*not positive definite.*frame 140"):
        ctx.graph_covariance([0], g["fixed"])
    # with 140 fixed as well the same store answers
    st, msg, out = raw_call(ctx, [1, 2, 140], [(0, 0), (5, 0), (140, 140)])
    assert st == 0 and np.all(np.diag(out[0].reshape(6, 6)) > 0.0) and np.all(out[2] == 0.0)
    # a cap below the order's work: the envelope solver's refusal
    _, prob = R.fixture("hub140")
    ea, eb = R.free_edges(dict(edges=g["edges"]), prob)
    _, _, stats = api.graph_order(prob.n_free, ea, eb)
    st, msg, out = raw_call(ctx, [1, 2, 140], [(0, 0)], max_work=stats["work"] - 1)
    assert st == -1 and f"velo_graph_covariance: the envelope solver's work is {stats['work']} block products, over the cap of {stats['work'] - 1} " in msg
    assert np.all(out == 7.0)
    with pytest.raises(api.VeloError, match=f"status -1.*work is {stats['work']} block products, over the cap of 1 .widest row {stats['widest_row']} "):
        ctx.graph_covariance([0], [1, 2, 140], max_work=1)
    st, msg, out = raw_call(ctx, [1, 2, 140], [(0, 0)], max_work=stats["work"])            # a cap the graph meets exactly is accepted
    assert st == 0
    # arguments
    for pairs, status, text in (([(0, 141)], -3, "frame 141, which has no pose"), ([(-1, 0)], -1, "frame"), ([(0, 1 << 22)], -1, "frame")):
        st, msg, out = raw_call(ctx, [1, 2, 140], pairs)
        assert st == status and text in msg and np.all(out == 7.0), (pairs, st, msg)
    one = np.zeros(1, dtype=np.int32)
    fx = np.asarray([1, 2, 140], dtype=np.int32)
    vp = lambda v: C.c_void_p(v.ctypes.data)                          # noqa: E731
    assert ctx._lib.velo_graph_covariance(ctx._h, vp(fx), 3, None, -1, vp(one), vp(one), vp(np.zeros(36))) == -1
    assert ctx._lib.velo_graph_covariance(ctx._h, vp(fx), 3, None, 1, None, vp(one), vp(np.zeros(36))) == -1
    assert ctx._lib.velo_graph_covariance(ctx._h, vp(fx), 3, None, 1, vp(one), vp(one), None) == -1
    assert ctx._lib.velo_graph_covariance(ctx._h, vp(fx), 3, None, 0, None, None, None) == 0
    with pytest.raises(api.VeloError, match="status -1.*ascending"):
        ctx.graph_covariance([0], [2, 1])
    assert state_bytes(ctx, g) == kept and ctx.graph_info()["optimizations"] == 0
    ctx.close()
