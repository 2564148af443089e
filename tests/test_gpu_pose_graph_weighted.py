"""velo_graph_add_edges_weighted / velo_graph_edge_stats against tests/pose_graph_weighted_ref.py, the numpy restatement of the pose
graph with a 6 x 6 information per edge and a Cauchy loss, on its fixtures: a pair and a chain of 5 with full information matrices,
a chain of 5 whose scalar odometry is promoted by a weighted loop edge with Cauchy, and a ring of 70 (two workgroups, edges shuffled
and added in two calls over one array growth) with three gross loop closures, with Cauchy and without.  The restatement's solves are
computed once per graph and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import pose_graph_ref as G
import pose_graph_weighted_ref as W
import velo_amd  # noqa: F401
from velo_amd import api

pytestmark = pytest.mark.gpu

# The spread between the restatement's two linear solvers, measured by tests/test_pose_graph_weighted_cpu.py (which says what an
# entry is where the two agree to below one unit of the format).  The kernels may differ from the restatement by 100 x that: the
# margin is for the summation order and the compiler's contraction.
SPREAD = {"pair_w": (2.3e-16, 8.9e-16), "chain5_w": (2.3e-16, 1.8e-15), "chain5_mixed": (3.3e-15, 8.9e-15),
          "ring70_outliers": (5.9e-14, 8.0e-14), "ring70_outliers_trivial": (5.7e-13, 1.7e-12)}
TOL = {k: (100.0 * c, 100.0 * x) for k, (c, x) in SPREAD.items()}
CHAIN5_TOL = 100.0 * 2.5e-14                                           # test_gpu_pose_graph.py: chain5's tolerance in the unknowns
SYSTEM_GATE = 1e-12                                                    # J^T J / J^T r against the largest entry
STATS_GATE = 1e-12                                                     # chi2 against the largest chi2, weights against 1
TERMINATION = {"gradient": 0, "parameter": 0, "function": 0, "radius": 0, "max_iterations": 1, "failure": 2}
LINEAR = {"cg": "pcg", "envelope": "direct"}


@functools.lru_cache(maxsize=None)
def reference(name, linear="pcg"):
    g = W.fixture(name)
    prob = W.problem_of(g)
    return g, prob, G.solve(prob, linear)


def add(ctx, edges):
    """consecutive edges of one kind in one call: a number as W goes through the scalar entry"""
    k = 0
    while k < len(edges):
        m = k
        while m < len(edges) and np.ndim(edges[m][3]) == np.ndim(edges[k][3]):
            m += 1
        part = edges[k:m]
        if np.ndim(part[0][3]) == 0:
            ctx.graph_add_edges([e[0] for e in part], [e[1] for e in part], [e[2] for e in part], [e[3] for e in part])
        else:
            ctx.graph_add_edges_weighted([e[0] for e in part], [e[1] for e in part], [e[2] for e in part], np.array([e[3] for e in part]),
                                         [e[4] for e in part])
        k = m


def load(ctx, g):
    ctx.graph_reset(g.get("edge_capacity", 0))
    frames = sorted(g["poses"])
    assert frames == list(range(len(frames)))
    ctx.graph_set_poses(0, np.array([g["poses"][k] for k in frames]))
    cut = g.get("split", len(g["edges"]))
    add(ctx, g["edges"][:cut])
    add(ctx, g["edges"][cut:])


def poses_of(ctx, g):
    return {f: ctx.graph_get_poses(f, 1)[0] for f in sorted(g["poses"])}


def state_bytes(ctx, g):
    return ctx.graph_get_poses(0, len(g["poses"])).tobytes()


def summary_bytes(s):
    return C.string_at(C.addressof(s), C.sizeof(s))


def as_solve(s, x):
    trace = [dict(status=t.status, cost=t.cost, candidate_cost=t.candidate_cost) for t in (s.trace[i] for i in range(s.n_trace))]
    return dict(trace=trace, initial_cost=s.initial_cost, final_cost=s.final_cost, x=x)


@pytest.mark.parametrize("name,solver", [(n, "cg") for n in W.FIXTURES] + [("ring70_outliers", "envelope"), ("chain5_w", "envelope")])
def test_solve_equals_the_restatement(name, solver):
    g, prob, want = reference(name, LINEAR[solver])
    ctx = api.Context(0)
    load(ctx, g)
    before = state_bytes(ctx, g)
    cost, gg, H = ctx.graph_system(g["fixed"])
    c0, g0, H0 = prob.system()
    e = (abs(cost - c0) / c0, np.max(np.abs(gg.ravel() - g0)) / np.max(np.abs(g0)), np.max(np.abs(H - H0)) / np.max(np.abs(H0)))
    print(f"{name}: cost {e[0]:.2e}, gradient {e[1]:.2e}, JtJ {e[2]:.2e} of the largest entry")
    assert max(e) <= SYSTEM_GATE
    chi2_0, weight_0 = ctx.graph_edge_stats()
    chi2_ref0, weight_ref0 = prob.edge_stats()
    es = (np.abs(chi2_0 - chi2_ref0).max() / chi2_ref0.max(), np.abs(weight_0 - weight_ref0).max())
    print(f"{name}: at the start chi2 {es[0]:.2e} of the largest, weights {es[1]:.2e}")
    assert max(es) <= STATS_GATE
    assert state_bytes(ctx, g) == before
    s = ctx.graph_optimize(g["fixed"], linear_solver=solver)
    after = poses_of(ctx, g)
    x = np.concatenate([after[f] for f in prob.free])
    got = as_solve(s, x)
    sc, sx = G.spread(got, want)
    print(f"{name}/{solver}: cost along the trace {sc:.3e} of the initial cost (tolerance {TOL[name][0]:.3e}), poses {sx:.3e} (tolerance {TOL[name][1]:.3e})")
    assert [t["status"] for t in got["trace"]] == [t["status"] for t in want["trace"]]
    assert s.termination == TERMINATION[want["termination"]]
    assert (s.iterations, s.evaluations, s.n_trace) == (want["iterations"], want["evaluations"], len(want["trace"]))
    assert (s.n_nodes, s.n_free, s.n_edges) == (prob.n_nodes, prob.n_free, prob.n_edges)
    assert sc <= TOL[name][0]
    assert sx <= TOL[name][1]
    # the edges' chi2 and weights at the stored -- now the final -- poses, whole and as a range
    chi2, weight = ctx.graph_edge_stats()
    chi2_ref, weight_ref = prob.edge_stats(x)
    # `pair_w` ends at cost 0: its one chi2 is then the square of a residual that is nothing but the rounding of the poses (1e-20, known
    # to no digit by whoever computes it -- pose_graph_ref.spread says the same of a cost near 0), so its scale is the start's chi2
    scale = chi2_ref0.max() if name == "pair_w" else chi2_ref.max()
    es = (np.abs(chi2 - chi2_ref).max() / scale, np.abs(weight - weight_ref).max())
    print(f"{name}/{solver}: chi2 {es[0]:.2e} of the largest, weights {es[1]:.2e}")
    assert max(es) <= STATS_GATE
    first, n = len(chi2) // 3, len(chi2) - len(chi2) // 3
    part = ctx.graph_edge_stats(first, n)
    assert part[0].tobytes() == chi2[first:].tobytes() and part[1].tobytes() == weight[first:].tobytes()
    assert state_bytes(ctx, g) == b"".join(after[f].tobytes() for f in sorted(after))
    if name == "pair_w":
        assert np.linalg.norm(after[1] - g["want"][1]) <= 1e-8 * (np.linalg.norm(g["want"][1]) + 1e-8)
        assert s.final_cost <= G.EPS * s.initial_cost
    if name == "chain5_mixed":
        assert 0.05 < weight[-1] < 0.95 and np.all(weight[:-1] == 1.0)
    if name.startswith("ring70"):
        info = ctx.graph_info()
        assert (info["n_nodes"], info["n_edges"], info["edge_reallocations"]) == (70, 274, 1) and info["edge_capacity"] >= 274
    ctx.close()


def test_cauchy_switches_gross_loop_closures_off():
    g, gt = W.fixture("ring70_outliers"), W.fixture("ring70_outliers_trivial")
    ctx = api.Context(0)
    load(ctx, g)
    ctx.graph_optimize(g["fixed"])
    robust, (_, weight) = poses_of(ctx, g), ctx.graph_edge_stats()
    load(ctx, gt)
    ctx.graph_optimize(gt["fixed"])
    trivial, (_, weight_trivial) = poses_of(ctx, gt), ctx.graph_edge_stats()
    ctx.close()
    out = g["outliers"]
    start, err, err_trivial = W.position_error(g, g["poses"]), W.position_error(g, robust), W.position_error(gt, trivial)
    print(f"outlier weights {weight[out]}, smallest other weight {np.delete(weight, out).min():.3f}; largest position error: start {start:.3f} m, "
          f"Cauchy {err:.3f} m, trivial {err_trivial:.3f} m")
    assert np.all(weight[out] < 1e-2)
    assert np.delete(weight, out).min() > 0.5
    assert err <= 0.25 * err_trivial
    assert err_trivial > start
    assert np.all(weight_trivial == 1.0)


def test_scalar_information_through_the_weighted_entry_is_the_scalar_path():
    g, gs = G.fixture("chain5"), W.fixture("chain5_scalar")
    ctx = api.Context(0)
    ctx.graph_reset()
    ctx.graph_set_poses(0, np.array([g["poses"][k] for k in range(5)]))
    ctx.graph_add_edges([e[0] for e in g["edges"]], [e[1] for e in g["edges"]], [e[2] for e in g["edges"]], [e[3] for e in g["edges"]])
    s = ctx.graph_optimize(g["fixed"])
    scalar = ctx.graph_get_poses(0, 5)
    load(ctx, gs)
    sw = ctx.graph_optimize(gs["fixed"])
    weighted = ctx.graph_get_poses(0, 5)
    ctx.close()
    assert [s.trace[k].status for k in range(s.n_trace)] == [sw.trace[k].status for k in range(sw.n_trace)]
    assert (s.termination, s.iterations, s.evaluations) == (sw.termination, sw.iterations, sw.evaluations)
    print(f"weighted entry against the scalar path: poses {np.abs(weighted - scalar).max():.2e} (tolerance {CHAIN5_TOL:.2e})")
    assert np.abs(weighted - scalar).max() <= CHAIN5_TOL


def scalar_ring70(ctx, stats=False):
    """ring70 through velo_graph_add_edges alone, as test_gpu_pose_graph.py loads it; the poses' and the summary's bytes"""
    g = G.fixture("ring70")
    ctx.graph_reset(64)
    ctx.graph_set_poses(0, np.array([g["poses"][k] for k in range(70)]))
    for part in (g["edges"][:g["split"]], g["edges"][g["split"]:]):
        ctx.graph_add_edges([e[0] for e in part], [e[1] for e in part], [e[2] for e in part], [e[3] for e in part])
    if stats:
        chi2, weight = ctx.graph_edge_stats()
        prob = G.problem_of(g)
        r = prob.evaluate(prob.x0(), False)[1].reshape(-1, 6)       # (sqrt(info) r: its square is info |r|^2)
        assert np.abs(chi2 - (r * r).sum(axis=1)).max() <= STATS_GATE * chi2.max() and np.all(weight == 1.0)
    s = ctx.graph_optimize(g["fixed"])
    return ctx.graph_get_poses(0, 70).tobytes() + summary_bytes(s)


def test_the_scalar_path_keeps_its_bytes():
    a = api.Context(0)
    first = scalar_ring70(a)
    b = api.Context(0)                                                # a weighted graph lives, and is solved, in another context
    g = W.fixture("ring70_outliers")
    load(b, g)
    b.graph_optimize(g["fixed"])
    second = scalar_ring70(a)
    c = api.Context(0)
    third = scalar_ring70(c)
    # ... and in the same context: velo_graph_reset returns the store to scalar-only
    load(a, g)
    a.graph_optimize(g["fixed"])
    fourth = scalar_ring70(a)
    # edge_stats on a scalar-only store answers info |r|^2 and 1, and leaves the next optimise as it was
    fifth = scalar_ring70(c, stats=True)
    for ctx in (a, b, c):
        ctx.close()
    assert first == second == third == fourth == fifth


def test_identical_calls_give_identical_bytes():
    g = W.fixture("ring70_outliers")
    out = []
    ctx = api.Context(0)
    for solver in ("cg", "cg", "envelope", "envelope"):
        load(ctx, g)
        s = ctx.graph_optimize(g["fixed"], linear_solver=solver)
        chi2, weight = ctx.graph_edge_stats()
        out.append(state_bytes(ctx, g) + summary_bytes(s) + chi2.tobytes() + weight.tobytes())
    ctx.close()
    assert out[0] == out[1] and out[2] == out[3]


def test_a_refused_weighted_call_changes_nothing():
    g = W.fixture("chain5_mixed")
    ctx = api.Context(0)
    load(ctx, g)
    kept, n_edges = state_bytes(ctx, g), ctx.graph_info()["n_edges"]
    z, eye = np.zeros(6), np.eye(6)
    bad_z, bad_w, indefinite, semi = z.copy(), eye.copy(), eye.copy(), eye.copy()
    bad_z[4], bad_w[2, 2], indefinite[3, 3], semi[5, 5] = np.nan, np.inf, -1.0, 0.0
    for args, text in ((([2], [2], [z], [eye]), "from == to"), (([0, -1], [1, 2], [z, z], [eye, eye]), "edge 1"), (([0], [1], [bad_z], [eye]), "z\\[4\\]"),
                       (([0], [1], [z], [bad_w]), "not finite"), (([0, 1], [1, 2], [z, z], [eye, indefinite]), "edge 1.*not positive definite"),
                       (([0], [1], [z], [semi]), "edge 0.*not positive definite"), (([0], [1], [z], [eye], [-1.0]), "loss_scale"),
                       (([0], [1], [z], [eye], [np.nan]), "loss_scale"), (([0], [1], [z], [eye], [np.inf]), "loss_scale")):
        with pytest.raises(api.VeloError, match="status -1.*" + text):
            ctx.graph_add_edges_weighted(*args)
    one = np.zeros(1, np.int32)
    assert ctx._lib.velo_graph_add_edges_weighted(ctx._h, 1, C.c_void_p(one.ctypes.data), C.c_void_p(one.ctypes.data), C.c_void_p(z.ctypes.data), None, None) == -1
    with pytest.raises(ValueError, match="not symmetric"):
        ctx.graph_add_edges_weighted([0], [1], [z], [eye + np.triu(np.ones((6, 6)), 1)])
    for first, n in ((-1, 1), (0, n_edges + 1), (n_edges, 1), (0, -1)):
        with pytest.raises(api.VeloError, match="status -1"):
            ctx.graph_edge_stats(first, n)
    assert len(ctx.graph_edge_stats(n_edges, 0)[0]) == 0
    assert state_bytes(ctx, g) == kept and ctx.graph_info()["n_edges"] == n_edges
    # the unchanged graph solves as a fresh copy of it does
    s = ctx.graph_optimize(g["fixed"])
    fresh = api.Context(0)
    load(fresh, g)
    sf = fresh.graph_optimize(g["fixed"])
    assert state_bytes(ctx, g) + summary_bytes(s) == state_bytes(fresh, g) + summary_bytes(sf)
    # an edge to a node without a pose is taken (the pose may still come) and stops edge_stats over it, not over the others
    ctx.graph_add_edges_weighted([0], [9], [z], [eye])
    with pytest.raises(api.VeloError, match="status -3"):
        ctx.graph_edge_stats()
    assert len(ctx.graph_edge_stats(0, n_edges)[0]) == n_edges
    other = api.Context(0)
    with pytest.raises(api.VeloError, match="status -3"):            # no velo_graph_reset on this context
        other.graph_edge_stats()
    with pytest.raises(api.VeloError, match="status -3"):
        other.graph_add_edges_weighted([0], [1], [z], [eye])
    for c in (ctx, fresh, other):
        c.close()
