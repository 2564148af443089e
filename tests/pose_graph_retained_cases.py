"""What tests/test_pose_graph_retained_cpu.py and tests/test_gpu_pose_graph_retained.py share: how each graph GROWS (a prefix, then
stages of new frames with the edges that become possible), what is asked at every grown state, and the numpy restatement of those
answers on top of pose_graph_cov_ref.py and pose_graph_gate_ref.py.  Test infrastructure only.

A stage's edges are the graph's edges, in the graph's order, whose later end arrives with the stage; `final(name)` is the whole graph
with its edges in the order the stages append them -- the order a context that loads it at once must use for its sums to have the terms
of the grown context's in the same sequence."""
import functools

import numpy as np

import pose_graph_cov_ref as R
import pose_graph_gate_ref as Q

GRAPHS = ("free1", "chain5", "chain12_tree", "chain250_split", "hub140", "ring70_open", "lap454_open")
# the graphs that grow: the frames of the prefix, then the frames each stage adds
GROWN = ("chain5", "ring70_open", "lap454_open", "chain250_split", "hub140")
# The states of a grown graph held against the NUMPY restatement: every one, but on chain250_split, whose 114 dense inverses of up to
# 1,482 unknowns would take most of a minute: there the prefix, every 16th state and the last.  Every state of every graph, chain250_split's
# included, is held to the bit against a context that loads that state whole (the GPU test's (b)).
CHECK_EVERY = {"chain5": 1, "ring70_open": 1, "hub140": 1, "chain250_split": 16, "lap454_open": 1}


def held_states(name):
    n = len(stages(name)[1])
    return [k for k in range(n) if name not in GROWN or k % CHECK_EVERY[name] == 0 or k == n - 1]


@functools.lru_cache(maxsize=None)
def stages(name):
    """(graph, [(frames, edges)]): stage 0 is the prefix"""
    g, _ = Q.fixture(name)
    frames = sorted(g["poses"])
    if name == "chain5":
        groups = [frames[:3]] + [[f] for f in frames[3:]]
    elif name == "ring70_open":
        groups = [frames[:40]] + [[f] for f in frames[40:]]
    elif name == "lap454_open":
        groups = [frames[:300]] + [frames[k:k + 22] for k in range(300, 454, 22)]
    elif name == "chain250_split":                                     # fixed 0, 125, 126: the first component is 1 .. 124
        groups = [frames[:137]] + [[f] for f in frames[137:]]
    elif name == "hub140":                                             # leaves 1 .. 130 around frame 0; frame 140 is fixed and has no edge
        groups = [[f for f in frames if f <= 110 or f == 140]] + [[f] for f in range(111, 131)]
    else:
        groups = [frames]
    assert sorted(f for grp in groups for f in grp) == frames and all(f in groups[0] for f in g["fixed"])
    posed, out, used = set(), [], [False] * len(g["edges"])
    for grp in groups:
        posed |= set(grp)
        new = [k for k, e in enumerate(g["edges"]) if not used[k] and e[0] in posed and e[1] in posed]
        for k in new:
            used[k] = True
        out.append((list(grp), [g["edges"][k] for k in new]))
    assert all(used)
    return g, out


def final(name):
    """the whole graph with its edges in the order the stages append them"""
    g, st = stages(name)
    return dict(g, edges=[e for _, edges in st for e in edges])


def state(name, k):
    """the graph after stage k: dict(poses, edges, fixed)"""
    g, st = stages(name)
    frames = [f for grp, _ in st[:k + 1] for f in grp]
    return dict(poses={f: g["poses"][f] for f in sorted(frames)}, edges=[e for _, edges in st[:k + 1] for e in edges], fixed=g["fixed"])


def free_graph(name, k):
    """(n_free, a, b): the free nodes of the state after stage k in ascending frame order and the edges between two of them, in free
    indices and in the state's edge order -- what the library hands to velo_graph_order_extend"""
    g, st = stages(name)
    frames = sorted(f for grp, _ in st[:k + 1] for f in grp if f not in g["fixed"])
    slot = {f: i for i, f in enumerate(frames)}
    pairs = [(slot[e[0]], slot[e[1]]) for _, edges in st[:k + 1] for e in edges if e[0] in slot and e[1] in slot]
    return len(frames), [p[0] for p in pairs], [p[1] for p in pairs]


def problem(name, gk, poses=None):
    _, prob = Q.fixture(name)
    return type(prob)(gk["poses"] if poses is None else poses, gk["edges"], gk["fixed"])


def requests(gk):
    """what is asked at a state: (cov pairs [n, 2], gate from, gate to, the candidates' query) -- every marginal, every edge's pair, pairs far
    apart in the order; the newest frame against frames spread over the graph (one column), and three pairs into another frame"""
    frames = sorted(gk["poses"])
    free = [f for f in frames if f not in gk["fixed"]]
    newest, oldest, mid = free[-1], free[0], free[len(free) // 2]
    pairs = [(f, f) for f in frames] + [(e[0], e[1]) for e in gk["edges"]] + [(oldest, newest), (newest, oldest), (mid, newest), (gk["fixed"][0], newest)]
    spread = sorted({free[(len(free) - 1) * j // 7] for j in range(8)} | {gk["fixed"][0]})
    frm = [f for f in spread if f != newest]
    to = [newest] * len(frm)
    if len(free) > 2:
        frm += [oldest, newest, free[1]]
        to += [mid, mid, mid] if mid not in (oldest, free[1]) else [free[-2], free[-2], free[-2]]
    keep = [k for k, (a, b) in enumerate(zip(frm, to)) if a != b]
    return (np.asarray(pairs, np.int32), np.asarray([frm[k] for k in keep], np.int32), np.asarray([to[k] for k in keep], np.int32), newest)


CAND = dict(min_gap=2, radius=3.0, k_sigma=3.0)


def restated(name, gk, poses):
    """(cov [n, 6, 6], gate (rel, r, S, chi2), candidates (frames, dist, sigma, margin), Sigma, problem) at `poses` by the dense inverse"""
    prob = problem(name, gk, poses)
    S = R.by_inverse(R.dense_jacobian(prob))
    return (*answers(S, prob, gk, poses), S, prob)


def answers(S, prob, gk, poses):
    pairs, frm, to, query = requests(gk)
    cov = np.array([Q.block(S, prob, int(a), int(b)) for a, b in pairs])
    gate = Q.gate(S, prob, poses, frm.tolist(), to.tolist())
    cand = Q.candidates(S, prob, poses, query, CAND["min_gap"], CAND["radius"], CAND["k_sigma"])
    return cov, gate, cand


def cov_spread(want, got, pairs, S, prob):
    """the largest |want - got| / (sigma_i sigma_j) over the blocks, sigma from Sigma's diagonal; a block with a fixed end must be zero"""
    worst = 0.0
    for (a, b), w, g in zip(pairs.tolist(), want, got):
        if a not in prob.slot or b not in prob.slot:
            assert np.all(g == 0.0), (a, b)
            continue
        sa = np.sqrt(np.diag(R.block_of(S, prob.slot[a], prob.slot[a])))
        sb = np.sqrt(np.diag(R.block_of(S, prob.slot[b], prob.slot[b])))
        worst = max(worst, R.cov_spread(w, g, sa, sb))
    return worst


def gate_spread(want, got, frm, to, fixed):
    worst = 0.0
    for p, (a, b) in enumerate(zip(frm.tolist(), to.tolist())):
        if a in fixed and b in fixed:
            continue
        worst = max(worst, Q.rel_spread(want[2][p], got[2][p]))
    return worst
