"""velo_graph_optimize / velo_graph_system against tests/pose_graph_ref.py, the numpy restatement of the pose-graph optimisation, on
the graphs of pose_graph_ref.fixture: a pair, a chain of 5 with a contradicting loop edge, a ring of 70 (two workgroups, edges
shuffled and added in two calls over two array growths), a hub with 130 spokes and two fixed nodes, and a chain whose global rotations
lie near pi.  The restatement's `pcg` solve is computed once per graph and shared."""
import ctypes as C
import functools

import numpy as np
import pytest

import pose_graph_ref as G
import velo_amd  # noqa: F401
from velo_amd import api

pytestmark = pytest.mark.gpu

# The spread between the restatement's two linear solvers (direct / block-Jacobi CG), measured by tests/test_pose_graph_cpu.py: in
# cost and candidate cost along the trace relative to the initial cost, absolute in the final unknowns (pose_graph_ref.spread says
# why the initial cost is the scale; `pair`, on which the two agree to the bit, has one unit of the format instead).  The kernels may
# differ from the restatement by 100 x that: the margin is for the summation order and the compiler's contraction.
SPREAD = {"pair": (2.3e-16, 8.9e-16), "chain5": (1.2e-15, 2.5e-14), "ring70": (1.4e-14, 7.7e-13), "hub": (8.5e-15, 2.0e-13),
          "large_rotation": (5.0e-14, 8.5e-14)}
TOL = {k: (100.0 * c, 100.0 * x) for k, (c, x) in SPREAD.items()}
SYSTEM_GATE = 1e-12                                                    # J^T J / J^T r against the largest entry
TERMINATION = {"gradient": 0, "parameter": 0, "function": 0, "radius": 0, "max_iterations": 1, "failure": 2}


@functools.lru_cache(maxsize=None)
def reference(name):
    g = G.fixture(name)
    prob = G.problem_of(g)
    return g, prob, G.solve(prob, "pcg")


def load(ctx, g, edge_capacity=0):
    """the graph into the context's store: runs of consecutive frames in one call each, the edges in one call or in two"""
    ctx.graph_reset(edge_capacity)
    frames = sorted(g["poses"])
    run = [frames[0]]
    for f in frames[1:] + [None]:
        if f is not None and f == run[-1] + 1:
            run.append(f)
            continue
        if len(run) == 1:
            ctx.graph_set_pose(run[0], g["poses"][run[0]])
        else:
            ctx.graph_set_poses(run[0], np.array([g["poses"][k] for k in run]))
        run = [f]
    cut = g.get("split", len(g["edges"]))
    for part in (g["edges"][:cut], g["edges"][cut:]):
        if part:
            ctx.graph_add_edges([e[0] for e in part], [e[1] for e in part], [e[2] for e in part], [e[3] for e in part])


def poses_of(ctx, g):
    return {f: ctx.graph_get_poses(f, 1)[0] for f in sorted(g["poses"])}


def state_bytes(ctx, g):
    return b"".join(p.tobytes() for p in poses_of(ctx, g).values())


def as_solve(s, x):
    trace = [dict(status=t.status, cost=t.cost, candidate_cost=t.candidate_cost, cg_iterations=t.cg_iterations, cg_residual=t.cg_residual)
             for t in (s.trace[i] for i in range(s.n_trace))]
    return dict(trace=trace, initial_cost=s.initial_cost, final_cost=s.final_cost, x=x)


@pytest.mark.parametrize("name", G.FIXTURES)
def test_solve_equals_the_restatement(name):
    g, prob, want = reference(name)
    ctx = api.Context(0)
    load(ctx, g, edge_capacity=64 if name == "ring70" else 0)
    before = poses_of(ctx, g)
    assert all(before[f].tobytes() == np.asarray(g["poses"][f], np.float64).tobytes() for f in before)
    # the system at the stored state
    cost, gg, H = ctx.graph_system(g["fixed"])
    c0, g0, H0 = prob.system()
    e = (abs(cost - c0) / c0, np.max(np.abs(gg.ravel() - g0)) / np.max(np.abs(g0)), np.max(np.abs(H - H0)) / np.max(np.abs(H0)))
    print(f"{name}: cost {e[0]:.2e}, gradient {e[1]:.2e}, JtJ {e[2]:.2e} of the largest entry")
    assert max(e) <= SYSTEM_GATE
    assert state_bytes(ctx, g) == b"".join(p.tobytes() for p in before.values())
    # the solve
    s = ctx.graph_optimize(g["fixed"])
    after = poses_of(ctx, g)
    got = as_solve(s, np.concatenate([after[f] for f in prob.free]))
    sc, sx = G.spread(got, want)
    print(f"{name}: cost along the trace {sc:.3e} of the initial cost (tolerance {TOL[name][0]:.3e}), poses {sx:.3e} (tolerance {TOL[name][1]:.3e}); "
          f"CG iterations {[t['cg_iterations'] for t in got['trace']]} (restatement {[t['cg_iterations'] for t in want['trace']]}), "
          f"residuals {[float('%.1e' % t['cg_residual']) for t in got['trace']]}")
    assert [t["status"] for t in got["trace"]] == [t["status"] for t in want["trace"]]
    assert s.termination == TERMINATION[want["termination"]]
    assert (s.iterations, s.evaluations, s.n_trace) == (want["iterations"], want["evaluations"], len(want["trace"]))
    assert (s.n_nodes, s.n_free, s.n_edges) == (prob.n_nodes, prob.n_free, prob.n_edges)
    assert sc <= TOL[name][0]
    assert sx <= TOL[name][1]
    assert all(after[f].tobytes() == before[f].tobytes() for f in g["fixed"])
    if name == "pair":                                               # T_0 . Z to the parameter tolerance; the final cost is 0
        assert np.linalg.norm(after[1] - g["want"][1]) <= 1e-8 * (np.linalg.norm(g["want"][1]) + 1e-8)
        assert s.final_cost <= G.EPS * s.initial_cost
    if name == "chain5":                                             # the loop edge's contradiction is spread over the chain
        moved = [np.linalg.norm(after[i][3:] - before[i][3:]) for i in range(1, 5)]
        assert all(m > 0.01 for m in moved) and moved[3] > moved[0]
    if name == "ring70":
        info = ctx.graph_info()
        assert (info["n_nodes"], info["n_edges"], info["edge_reallocations"], info["optimizations"]) == (70, 271, 2, 1) and info["edge_capacity"] >= 271
        assert s.final_cost < 0.01 * s.initial_cost
    if name == "hub":                                                # a free node without edges keeps its bytes
        assert after[140].tobytes() == before[140].tobytes() and s.n_free == 130
        assert sum(1 for a, b, _, _ in g["edges"] if 0 in (a, b)) > 128     # the hub's degree: 130 spokes and the duplicate of one
    if name == "large_rotation":
        assert min(np.linalg.norm(p[:3]) for p in after.values()) > 3.0
    ctx.close()


def test_identical_calls_give_identical_bytes():
    g, _, _ = reference("ring70")
    out = []
    ctx = api.Context(0)
    for _ in range(2):
        load(ctx, g, edge_capacity=64)
        s = ctx.graph_optimize(g["fixed"])
        out.append(state_bytes(ctx, g) + C.string_at(C.addressof(s), C.sizeof(s)))
    assert out[0] == out[1]
    # a converged graph: the first iteration ends the solve and no pose moves
    kept = state_bytes(ctx, g)
    s = ctx.graph_optimize(g["fixed"])
    assert s.iterations == 1 and s.termination == 0 and s.trace[0].status in (api.BA_PARAMETER, api.BA_FUNCTION)
    assert state_bytes(ctx, g) == kept
    ctx.close()


def test_a_refused_call_changes_nothing():
    g, _, _ = reference("chain5")
    ctx = api.Context(0)
    load(ctx, g)
    kept, n_edges = state_bytes(ctx, g), ctx.graph_info()["n_edges"]
    z = np.zeros(6)
    bad_z = z.copy()
    bad_z[4] = np.nan
    for args in (([2], [2], [z], [1.0]), ([0], [1], [z], [0.0]), ([0], [1], [z], [-1.0]), ([0], [1], [z], [np.inf]), ([0], [1], [bad_z], [1.0]),
                 ([0, -1], [1, 2], [z, z], [1.0, 1.0])):
        with pytest.raises(api.VeloError, match="status -1"):
            ctx.graph_add_edges(*args)
    for fixed in ([], [1, 0], [0, 0]):
        with pytest.raises(api.VeloError, match="status -1"):     # no fixed node; not ascending; not distinct
            ctx.graph_optimize(fixed)
    with pytest.raises(api.VeloError, match="status -3"):         # a fixed frame without a pose
        ctx.graph_optimize([7])
    with pytest.raises(api.VeloError, match="status -3"):
        ctx.graph_get_poses(3, 4)
    with pytest.raises(api.VeloError, match="status -1"):
        ctx.graph_set_pose(1, bad_z)
    assert state_bytes(ctx, g) == kept and ctx.graph_info()["n_edges"] == n_edges
    # an edge to a node without a pose is taken (the pose may still come) and stops the solve
    ctx.graph_add_edges([0], [9], [z], [1.0])
    with pytest.raises(api.VeloError, match="status -3"):
        ctx.graph_optimize(g["fixed"])
    with pytest.raises(api.VeloError, match="status -3"):
        ctx.graph_system(g["fixed"])
    assert state_bytes(ctx, g) == kept
    other = api.Context(0)
    with pytest.raises(api.VeloError, match="status -3"):         # no velo_graph_reset on this context
        other.graph_set_pose(0, z)
    other.close()
    ctx.close()
