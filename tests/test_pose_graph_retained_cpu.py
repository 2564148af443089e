"""What of velo_graph_retain needs no GPU: velo_graph_order_extend, the rule for the order of a graph that has grown, against
tests/graph_order_extend_ref.py (the header's rule restated in pure Python); the header's constants and the refusals of the three
entries without a context; and SPREAD_REL, what the numpy restatement's own routes differ by at the grown states that
tests/test_gpu_pose_graph_retained.py holds the kernels to."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import graph_order_extend_ref as X
import graph_order_ref as O
import pose_graph_cov_ref as R
import pose_graph_gate_ref as Q
import pose_graph_retained_cases as K
import velo_amd  # noqa: F401
from test_graph_order_cpu import GRAPHS
from velo_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BIG = 1 << 24

# Measured here, recorded as measured, over the states the GPU test holds against numpy (K.held_states: EVERY state of chain5, ring70_open,
# hub140 and lap454_open; of chain250_split's 114 the prefix, every 16th and the last) and the requests of K.requests: "<graph>/cov" the
# largest difference of a covariance block between Sigma by the inverse and Sigma by the QR of J and -- at the LAST state of every graph
# only, the one state whose order the restatement's Takahashi route is run for -- inside the envelope the Takahashi route, in units of
# sigma_i sigma_j; "<graph>" the same between the inverse and the QR route for Sigma_rel of the gate's pairs.
SPREAD_REL = {"free1": 2.2e-16, "free1/cov": 2.6e-16, "chain5": 1.2e-15, "chain5/cov": 1.5e-15, "chain12_tree": 2.1e-10, "chain12_tree/cov": 2.4e-11,
              "chain250_split": 4.7e-11, "chain250_split/cov": 5.6e-11, "hub140": 6.6e-14, "hub140/cov": 2.7e-13, "ring70_open": 5.0e-14,
              "ring70_open/cov": 9.9e-14, "lap454_open": 1.8e-12, "lap454_open/cov": 3.3e-12}


@pytest.fixture(scope="module", autouse=True)
def lib():
    build.build_hip()
    return api.load_library()


def grow(n, a, b, sizes, hold=lambda u, v: False):
    """[(n_k, a_k, b_k, first_new_edge)]: the graph on the nodes 0 .. n_k - 1 for every size, an edge arriving with its later end, the old
    edges first; a last step adds the edges `hold` kept back"""
    out, ea, eb, used = [], [], [], [False] * len(a)
    for nk in sizes:
        first_new = len(ea)
        for e, (u, v) in enumerate(zip(a, b)):
            if not used[e] and u < nk and v < nk and not hold(u, v):
                used[e] = True
                ea.append(u)
                eb.append(v)
        out.append((nk, list(ea), list(eb), first_new))
    if not all(used):
        first_new = len(ea)
        ea += [u for e, u in enumerate(a) if not used[e]]
        eb += [v for e, v in enumerate(b) if not used[e]]
        out.append((sizes[-1], ea, eb, first_new))
    return out


def growths():
    n, a, b = GRAPHS["star131"]
    return {
        "path5": grow(*GRAPHS["path5"], [3, 4, 5]),
        "ring70": grow(*GRAPHS["ring70"], list(range(40, 71)), hold=lambda u, v: abs(u - v) > 4),
        "star131": grow(n, a, b, list(range(18, 132))),                # the hub is node 17
        "two_components_and_a_loner": grow(*GRAPHS["two_components_and_a_loner"], [4, 6, 7, 8, 9]),
        "lap454": grow(*GRAPHS["lap454"], list(range(300, 454, 22)) + [454]),
    }


def run(steps, max_work=BIG, perm0=None):
    """the library and the restatement side by side through the steps, each from the library's previous order; the stats of every step"""
    n_old, perm_old, first_old, seen = 0, np.zeros(0, np.int32), None, []
    if perm0 is not None:
        n_old, perm_old = len(perm0), np.asarray(perm0, np.int32)
    for nk, a, b, first_new in steps:
        first_new = first_new if n_old else 0
        perm, first, stats = api.graph_order_extend(n_old, perm_old, nk, a, b, first_new, max_work)
        wp, wf, ws = X.order_extend(n_old, perm_old.tolist(), nk, a, b, first_new, max_work)
        assert perm.tolist() == wp.tolist() and first.tolist() == wf.tolist()
        assert tuple(stats.values()) == tuple(int(v) for v in ws), (stats, ws)
        assert sorted(perm.tolist()) == list(range(nk))
        nb = O.neighbours(nk, a, b)
        by_definition, (widest, blocks, work) = O.stats_of(nb, perm)
        assert first.tolist() == by_definition.tolist() and (stats["widest_row"], stats["envelope_blocks"], stats["work"]) == (widest, blocks, work)
        p = stats["first_dirty_row"]
        if not stats["rebuilt"]:
            assert perm[:n_old].tolist() == perm_old.tolist() and perm[n_old:].tolist() == list(range(n_old, nk))
            pos = {int(v): k for k, v in enumerate(perm)}
            touched = [pos[v] for e in range(first_new, len(a)) for v in (a[e], b[e])] + ([n_old] if n_old < nk else [])
            assert p == (min(touched) if touched else nk)              # the smallest touched position
            if first_old is not None:
                assert first[:min(p, n_old)].tolist() == first_old[:min(p, n_old)].tolist()      # the rows before it keep their first
            assert work <= max_work and work <= X.RATIO * stats["fresh_work"] and stats["reversed"] == 0
        else:
            assert p == 0
        seen.append(stats)
        n_old, perm_old, first_old = nk, perm, first
    return seen


@pytest.mark.parametrize("name", sorted(growths()))
def test_order_extend_equals_the_restatement(name):
    seen = run(growths()[name])
    rebuilt = [k for k, s in enumerate(seen) if s["rebuilt"]]
    print(f"{name}: {len(seen)} steps, rebuilds at {rebuilt}; work {seen[-1]['work']} against the fresh order's {seen[-1]['fresh_work']}; first dirty rows {[s['first_dirty_row'] for s in seen][:12]}")
    if name == "ring70":                                               # the closing edges join the two ends of the order
        assert seen[-1]["rebuilt"] == 1 and not any(s["rebuilt"] for s in seen[1:-1])


def test_nothing_new_leaves_every_row():
    n, a, b = GRAPHS["lap454"]
    perm, first, _ = api.graph_order(n, a, b)
    p2, f2, stats = api.graph_order_extend(n, perm, n, a, b, len(a))
    assert stats["first_dirty_row"] == n and stats["rebuilt"] == 0 and p2.tolist() == perm.tolist() and f2.tolist() == first.tolist()
    assert stats["work"] == stats["fresh_work"] or stats["work"] <= X.RATIO * stats["fresh_work"]


def test_the_cap_both_ratio_branches_and_both_orientations():
    chain = lambda n: (n, list(range(n - 1)), list(range(1, n)))       # noqa: E731
    flags = set()
    # the ratio holds and the cap holds: kept.  The frame order of a chain is as good as any
    s = run([(*chain(10), 0)])[0]
    assert (s["rebuilt"], s["work"], s["fresh_work"]) == (0, 9, 9)
    # the cap alone fails: the fresh order, whose work the caller then compares.  velo_graph_order puts a chain's last node FIRST; reversed,
    # it comes last
    s = run([(*chain(10), 0)], max_work=8)[0]
    assert (s["rebuilt"], s["reversed"], s["work"]) == (1, 1, 9)
    flags.add((s["rebuilt"], s["reversed"]))
    perm, _, _ = api.graph_order_extend(0, [], *chain(10), 0, 8)
    assert perm.tolist() == list(range(10)) and api.graph_order(*chain(10))[0].tolist() == list(range(9, -1, -1))
    # the ratio alone fails: ring70's closing edges on the frame order
    n, a, b = GRAPHS["ring70"]
    s = run([(n, a, b, 0)], perm0=None)[0]
    assert s["rebuilt"] == 1 and s["work"] <= BIG
    flags.add((s["rebuilt"], s["reversed"]))
    # the highest node in the middle of the fresh order: no reversal helps
    s = run([(*GRAPHS["path5"], 0)], max_work=0)[0]
    assert (s["rebuilt"], s["reversed"]) == (1, 0)
    flags.add((s["rebuilt"], s["reversed"]))
    # a reversal that is refused for its work: star131's fresh order starts with the highest leaf (position 0: the first half) and ends
    # leaves, hub, leaf; reversed, every leaf's row would reach back to the hub at position 1 -- 366,146 block products against 8,386
    n, a, b = GRAPHS["star131"]
    perm, _, fresh = api.graph_order(n, a, b)
    at = int(np.nonzero(perm == n - 1)[0][0])
    _, (_, _, back_work) = O.stats_of(O.neighbours(n, a, b), perm[::-1].copy())
    assert 2 * at < n and 2 * (n - 1 - at) >= n and back_work > X.RATIO * fresh["work"]
    s = run([(n, a, b, 0)], max_work=0)[0]
    assert (s["rebuilt"], s["reversed"], s["work"]) == (1, 0, fresh["work"])
    assert {(1, 1), (1, 0)} <= flags


def test_refusals_of_order_extend():
    ok = dict(n_old=3, perm_old=[2, 0, 1], n_nodes=5, a=[0, 1, 2, 3], b=[1, 2, 3, 4], first_new_edge=2)
    assert api.graph_order_extend(**ok)[2]["first_dirty_row"] == 0     # node 2 sits at position 0 and the new edge (2, 3) ends there
    for change, text in ((dict(perm_old=[2, 0, 0]), "not a permutation"), (dict(perm_old=[3, 0, 1]), "not a permutation"), (dict(b=[1, 2, 3, 5]), "joins 3 and 5"),
                         (dict(a=[0, 1, 2, 4]), "a == b"), (dict(first_new_edge=5), "first_new_edge"), (dict(first_new_edge=3), "ends at a new node"),
                         (dict(n_nodes=2), "n_old <= n_nodes"), (dict(max_work=-1), "negative max_work")):
        with pytest.raises(api.VeloError, match="status -1.*velo_graph_order_extend.*" + text):
            api.graph_order_extend(**dict(ok, **change))
    lib = api.load_library()
    three = (C.c_int32 * 5)(2, 0, 1, 0, 0)
    stats = (C.c_int64 * 8)()
    vp = lambda v: C.cast(v, C.c_void_p)                               # noqa: E731
    assert lib.velo_graph_order_extend(3, None, 3, 0, None, None, 0, BIG, vp(three), vp(three), vp(stats)) == -1
    assert lib.velo_graph_order_extend(3, vp(three), 3, 0, None, None, 0, BIG, None, vp(three), vp(stats)) == -1
    assert lib.velo_graph_order_extend(3, vp(three), 3, 1, None, vp(three), 0, BIG, vp(three), vp(three), vp(stats)) == -1
    out = (C.c_int32 * 3)()
    assert lib.velo_graph_order_extend(3, vp(three), 3, 0, None, None, 0, BIG, vp(out), vp(three), vp(stats)) == 0 and list(out) == [2, 0, 1]


def test_header_constants_and_the_entries_without_a_context():
    with open(os.path.join(ROOT, "include", "velo_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define VELO_GRAPH_RETAIN_REBUILD_RATIO 2\b", header) and X.RATIO == 2
    for name in ("velo_graph_retain", "velo_graph_release", "velo_graph_retained", "velo_graph_order_extend"):
        assert re.search(r"\bint " + name + r"\(", header), name
    assert "int64_t info[16]" in header
    lib = api.load_library()
    one = (C.c_int32 * 1)(0)
    info = (C.c_int64 * 16)(*([7] * 16))
    vp = lambda v: C.cast(v, C.c_void_p)                               # noqa: E731
    assert lib.velo_graph_retain(None, vp(one), 1, None, None, 0) == -1 and b"null ctx" in lib.velo_last_error()
    assert lib.velo_graph_release(None) == -1 and b"null ctx" in lib.velo_last_error()
    assert lib.velo_graph_retained(None, vp(info), None, 0) == -1 and b"null ctx" in lib.velo_last_error()
    assert list(info) == [7] * 16
    keys = ("state", "n_free", "widest_row", "blocks", "work", "builds", "extensions", "rebuilds", "selected_inverses", "columns", "served", "first_dirty_row",
            "rows_refactored")
    assert len(keys) == 13 and "[13..15] 0" in header


@functools.lru_cache(maxsize=None)
def rule_through_stages(name):
    """the stats of velo_graph_order_extend for the free graph of every state of a grown fixture, from the frame order of the prefix"""
    g, st = K.stages(name)
    perm, n_old, m_old, seen = np.zeros(0, np.int32), 0, 0, []
    for k in range(len(st)):
        n, ea, eb = K.free_graph(name, k)
        perm, first, stats = api.graph_order_extend(n_old, perm, n, ea, eb, m_old if k else 0)
        seen.append(stats)
        n_old, m_old = n, len(ea)
    return seen


# the stages of the GPU test's growths at which the rule says rebuild: chain250_split's loop edge (130, 247) arrives with frame 247 and would
# make a row of 117 blocks at the end of the frame order; the fresh order of the closed loop does not end at the newest frame, so the two
# appends after it rebuild as well -- what the ratio of 2 costs once a loop is closed
REBUILDS = {"chain250_split": [111, 112, 113]}


def test_the_gpu_tests_growths_extend():
    """what test (b) on the GPU counts on: the growths are extensions, but for the one loop edge"""
    for name in K.GROWN:
        seen = rule_through_stages(name)
        print(f"{name}: {len(seen)} states; the prefix {'rebuilt' if seen[0]['rebuilt'] else 'in frame order'}; work {seen[-1]['work']} against the fresh order's {seen[-1]['fresh_work']}")
        assert [k for k, s in enumerate(seen) if k and s["rebuilt"]] == REBUILDS.get(name, []), name
        assert any(s["first_dirty_row"] > 0 for s in seen[1:])         # (chain5's frame 3 has an edge to frame 1, which is row 0)


@functools.lru_cache(maxsize=None)
def spreads(name):
    """("<name>/cov", "<name>") over the states the GPU test checks"""
    g, st = K.stages(name)
    cov_worst = rel_worst = 0.0
    for k in range(len(st)):
        if k not in K.held_states(name):
            continue
        gk = K.state(name, k)
        prob = K.problem(name, gk)
        poses = prob.poses_of(prob.x0())
        J = R.dense_jacobian(prob)
        S1, S2 = R.by_inverse(J), R.by_qr(J)
        pairs, frm, to, query = K.requests(gk)
        c1, g1, _ = K.answers(S1, prob, gk, poses)
        c2, g2, _ = K.answers(S2, prob, gk, poses)
        cov_worst = max(cov_worst, K.cov_spread(c1, c2, pairs, S1, prob))
        rel_worst = max(rel_worst, K.gate_spread(g1, g2, frm, to, gk["fixed"]))
        if k == len(st) - 1:                                           # the Takahashi route, inside its envelope, at the last state
            ea, eb = R.free_edges(gk, prob)
            T = R.Takahashi(J, prob.n_free, ea, eb)
            inside = [(a, b) for a, b in pairs.tolist() if a in prob.slot and b in prob.slot and T.inside(prob.slot[a], prob.slot[b])]
            c3 = np.array([T.block(prob.slot[a], prob.slot[b]) for a, b in inside])
            c1i = np.array([Q.block(S1, prob, a, b) for a, b in inside])
            cov_worst = max(cov_worst, K.cov_spread(c1i, c3, np.asarray(inside), S1, prob))
            assert T.outside_reads == 0
    return cov_worst, rel_worst


@pytest.mark.parametrize("name", K.GRAPHS)
def test_the_routes_agree_at_the_grown_states(name):
    cov, rel = spreads(name)
    print(f"{name}: covariance blocks {cov:.2e} (record {SPREAD_REL[name + '/cov']:.1e}); Sigma_rel {rel:.2e} (record {SPREAD_REL[name]:.1e})")
    assert cov <= 3 * SPREAD_REL[name + "/cov"] and rel <= 3 * SPREAD_REL[name]      # the record is what was measured, to a factor of 3 (LAPACK builds differ)
