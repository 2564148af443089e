"""velo_graph_optimize with the envelope solver (linear_solver="envelope": an exact block-skyline Cholesky in the order of
velo_graph_order) against the `direct` solve of tests/pose_graph_ref.py, the numpy restatement: on the five graphs of
pose_graph_ref.FIXTURES and on the five of tests/pose_graph_env_fixtures.py, which are chosen for where the factorisation can go
wrong.  The restatement is solved once per graph and shared.  The two solvers are told apart by cg_iterations == 0 and by the
envelope's figures in graph_info."""
import ctypes as C
import functools

import numpy as np
import pytest

import pose_graph_env_fixtures as F
import pose_graph_ref as G
import velo_amd  # noqa: F401
from velo_amd import api

pytestmark = pytest.mark.gpu

# The spread between the restatement's two linear solvers (direct / block-Jacobi CG): cost and candidate cost along the trace relative
# to the initial cost, the final unknowns in absolute terms.  The first five are the numbers of tests/test_gpu_pose_graph.py (SPREAD,
# measured by tests/test_pose_graph_cpu.py); the others are measured by tests/test_graph_order_cpu.py (SPREAD), with CG run to its
# tolerance in every LM iteration.  The kernels may differ from the restatement by 100 x that: the project's margin for the summation
# order and the compiler's contraction.
SPREAD = {"pair": (2.3e-16, 8.9e-16), "chain5": (1.2e-15, 2.5e-14), "ring70": (1.4e-14, 7.7e-13), "hub": (8.5e-15, 2.0e-13),
          "large_rotation": (5.0e-14, 8.5e-14),
          "chain250": (3.3e-13, 4.5e-11), "chain250_split": (2.9e-13, 4.4e-12), "lap454": (2.1e-11, 2.9e-9), "free1": (2.3e-16, 4.5e-16),
          "free2": (8.8e-15, 3.2e-15)}
TOL = {k: (100.0 * c, 100.0 * x) for k, (c, x) in SPREAD.items()}
TERMINATION = {"gradient": 0, "parameter": 0, "function": 0, "radius": 0, "max_iterations": 1, "failure": 2}
ALL = G.FIXTURES + F.ENV_FIXTURES


@functools.lru_cache(maxsize=None)
def reference(name):
    g = G.fixture(name) if name in G.FIXTURES else F.fixture(name)
    prob = G.problem_of(g)
    return g, prob, G.solve(prob, "direct")


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
    frames = sorted(g["poses"])
    out = {}
    for f in frames:                                                   # (one call per run would do; the graphs are small)
        out[f] = ctx.graph_get_poses(f, 1)[0]
    return out


def state_bytes(ctx, g):
    return b"".join(p.tobytes() for p in poses_of(ctx, g).values())


def summary_bytes(s):
    return C.string_at(C.addressof(s), C.sizeof(s))


def as_solve(s, x):
    trace = [dict(status=t.status, cost=t.cost, candidate_cost=t.candidate_cost) for t in (s.trace[i] for i in range(s.n_trace))]
    return dict(trace=trace, initial_cost=s.initial_cost, final_cost=s.final_cost, x=x)


@pytest.mark.parametrize("name", ALL)
def test_envelope_solve_equals_the_direct_restatement(name):
    g, prob, want = reference(name)
    ctx = api.Context(0)
    load(ctx, g, edge_capacity=64 if name == "ring70" else 0)
    before = poses_of(ctx, g)
    info = ctx.graph_info()
    assert (info["envelope_widest_row"], info["envelope_blocks"]) == (0, 0)      # until there has been an envelope solve
    s = ctx.graph_optimize(g["fixed"], linear_solver="envelope")
    after = poses_of(ctx, g)
    got = as_solve(s, np.concatenate([after[f] for f in prob.free]))
    sc, sx = G.spread(got, want)
    n, ea, eb = F.free_graph(g)
    _, _, stats = api.graph_order(n, ea, eb)
    info = ctx.graph_info()
    print(f"{name}: cost along the trace {sc:.3e} of the initial cost (tolerance {TOL[name][0]:.3e}), poses {sx:.3e} (tolerance {TOL[name][1]:.3e}); "
          f"statuses {[t['status'] for t in got['trace']]}; widest row {stats['widest_row']}, envelope {stats['envelope_blocks']} blocks, work {stats['work']}, "
          f"{stats['components']} components")
    assert [t["status"] for t in got["trace"]] == [t["status"] for t in want["trace"]]
    assert s.termination == TERMINATION[want["termination"]]
    assert (s.iterations, s.evaluations, s.n_trace) == (want["iterations"], want["evaluations"], len(want["trace"]))
    assert (s.n_nodes, s.n_free, s.n_edges) == (prob.n_nodes, prob.n_free, prob.n_edges)
    assert (info["n_nodes"], info["n_edges"], info["optimizations"]) == (prob.n_nodes, prob.n_edges, 1)
    assert sc <= TOL[name][0]
    assert sx <= TOL[name][1]
    assert s.n_trace >= 2 and all(s.trace[i].cg_iterations == 0 and s.trace[i].cg_residual == 0.0 for i in range(s.n_trace))
    assert all(after[f].tobytes() == before[f].tobytes() for f in g["fixed"])
    assert (info["envelope_widest_row"], info["envelope_blocks"]) == (stats["widest_row"], stats["envelope_blocks"])
    if name == "hub":                                                # a free node without edges keeps its bytes; the hub's row holds
        assert after[140].tobytes() == before[140].tobytes() and s.n_free == 130      # 128 blocks (127 leaves and itself): two waves' worth
        assert stats["widest_row"] + 1 >= 128 and stats["components"] == 2
    if name == "chain250":
        assert s.final_cost < 0.5 * s.initial_cost
    if name == "chain250_split":
        assert stats["components"] == 2
    if name == "lap454":
        assert s.final_cost < 0.01 * s.initial_cost and stats["widest_row"] >= 20
    ctx.close()


def test_the_cg_cap_is_ignored_by_the_envelope_solver():
    g, _, _ = reference("chain250")
    ctx = api.Context(0)
    out = []
    for kw in (dict(linear_solver="envelope"), dict(linear_solver="envelope", cg_max_iterations=5), dict(cg_max_iterations=5)):
        load(ctx, g)
        s = ctx.graph_optimize(g["fixed"], **kw)
        out.append(state_bytes(ctx, g) + summary_bytes(s))
    assert out[0] == out[1]
    assert out[2] != out[0]                                           # the CG with that cap stops short
    ctx.close()


def test_identical_calls_give_identical_bytes_and_the_cg_path_is_untouched():
    g, _, _ = reference("ring70")
    ctx = api.Context(0)
    out = []
    for _ in range(2):
        load(ctx, g, edge_capacity=64)
        s = ctx.graph_optimize(g["fixed"], linear_solver="envelope")
        out.append(state_bytes(ctx, g) + summary_bytes(s))
    assert out[0] == out[1]
    # a converged graph: the first iteration ends the solve and no pose moves
    kept = state_bytes(ctx, g)
    s = ctx.graph_optimize(g["fixed"], linear_solver="envelope")
    assert s.iterations == 1 and s.termination == 0 and s.trace[0].status in (api.BA_PARAMETER, api.BA_FUNCTION) and s.trace[0].cg_iterations == 0
    assert state_bytes(ctx, g) == kept
    # a CG call after envelope calls on the same context gives the bytes a fresh context's CG call gives
    load(ctx, g, edge_capacity=64)
    s = ctx.graph_optimize(g["fixed"])
    used = state_bytes(ctx, g) + summary_bytes(s)
    fresh_ctx = api.Context(0)
    load(fresh_ctx, g, edge_capacity=64)
    s2 = fresh_ctx.graph_optimize(g["fixed"])
    assert used == state_bytes(fresh_ctx, g) + summary_bytes(s2)
    assert s.trace[0].cg_iterations > 0
    fresh_ctx.close()
    ctx.close()


def test_a_refused_call_changes_nothing():
    g, _, _ = reference("ring70")
    ctx = api.Context(0)
    load(ctx, g)
    kept = state_bytes(ctx, g)
    n, ea, eb = F.free_graph(g)
    _, _, stats = api.graph_order(n, ea, eb)
    assert stats["work"] > 1
    with pytest.raises(api.VeloError, match="status -1.*linear solver 2"):
        ctx.graph_optimize(g["fixed"], linear_solver=2)
    assert state_bytes(ctx, g) == kept
    with pytest.raises(api.VeloError, match=f"status -1.*work is {stats['work']} block products, over the cap of 1 .widest row {stats['widest_row']} "):
        ctx.graph_optimize(g["fixed"], linear_solver="envelope", max_work=1)
    assert state_bytes(ctx, g) == kept
    for solver in ("envelope", "cg"):
        with pytest.raises(api.VeloError, match="status -1.*negative work cap"):
            ctx.graph_optimize(g["fixed"], linear_solver=solver, max_work=-1)
        assert state_bytes(ctx, g) == kept
    info = ctx.graph_info()
    assert (info["optimizations"], info["envelope_widest_row"], info["envelope_blocks"]) == (0, 0, 0)
    # a cap the graph meets exactly is accepted
    s = ctx.graph_optimize(g["fixed"], linear_solver="envelope", max_work=stats["work"])
    assert s.termination == 0 and state_bytes(ctx, g) != kept
    ctx.close()
