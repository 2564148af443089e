"""velo_graph_retain: the factorisation velo_graph_covariance, velo_graph_edge_gate and velo_graph_loop_candidates build, kept between
calls and extended on append.  What is held to what:

  (a) retained in api.graph_order's order, every answer is an un-retained context's TO THE BIT; the counters show what was skipped
  (b) a context that grows (retain a prefix, append, ask, append, ...) gives at EVERY state the bits of one that loads that state whole and
      retains in the grown context's order of that state: the partial factorisation equals the full one
  (c) the grown states against the numpy restatement within 100 x SPREAD_REL of tests/test_pose_graph_retained_cpu.py: every state, but on
      chain250_split the prefix, every 16th state and the last (K.held_states)
  (d) ring70_open's closing edge (an extension: its other end is fixed), closing edges between free frames (a rebuild); the held edges
      gate as tests/test_gpu_pose_graph_gate.py records
  (e) what drops the state, (f) a new frame without an edge, (g) asking changes nothing a solve sees
  (h) the three kinds of query in another order, with sizes that shrink and grow between them: every answer a fresh context's
"""
import numpy as np
import pytest

import pose_graph_gate_ref as Q
import pose_graph_retained_cases as K
import velo_amd  # noqa: F401
from test_gpu_pose_graph_covariance import load, poses_of, state_bytes, summary_bytes
from test_pose_graph_retained_cpu import SPREAD_REL, rule_through_stages
from velo_amd import api

pytestmark = pytest.mark.gpu

TOL = {k: 100.0 * v for k, v in SPREAD_REL.items()}


def add_edges(ctx, edges):
    """a stage's edges, as test_gpu_pose_graph_covariance.load adds a run of one kind"""
    if not edges:
        return
    if np.ndim(edges[0][3]) == 0:
        ctx.graph_add_edges([e[0] for e in edges], [e[1] for e in edges], [e[2] for e in edges], [e[3] for e in edges])
    else:
        ctx.graph_add_edges_weighted([e[0] for e in edges], [e[1] for e in edges], [e[2] for e in edges], np.array([e[3] for e in edges]), [e[4] for e in edges])


def append(ctx, g, stage):
    frames, edges = stage
    for f in frames:
        ctx.graph_set_pose(f, g["poses"][f])
    add_edges(ctx, edges)


def ask(ctx, gk):
    """(cov, gate, candidates) of K.requests at the context's state"""
    pairs, frm, to, query = K.requests(gk)
    cov = ctx.graph_covariance(pairs, gk["fixed"])
    gate = ctx.graph_edge_gate(frm, to, None, None, gk["fixed"])
    cand = ctx.graph_loop_candidates(query, K.CAND["min_gap"], K.CAND["radius"], K.CAND["k_sigma"], gk["fixed"], capacity=512)
    return cov, gate, cand


def as_bytes(ans):
    cov, gate, cand = ans
    return cov.tobytes() + b"".join(x.tobytes() for x in gate) + b"".join(x.tobytes() for x in cand)


def library_perm(name, gk):
    prob = K.problem(name, gk)
    ea, eb = Q.R.free_edges(gk, prob)
    return api.graph_order(prob.n_free, ea, eb)[0]


@pytest.mark.parametrize("name", K.GRAPHS)
def test_a_retained_in_the_librarys_order_every_answer_keeps_its_bytes(name):
    gk = K.final(name)
    kept, plain = api.Context(0), api.Context(0)
    load(kept, gk)
    load(plain, gk)
    kept.graph_retain(gk["fixed"], perm=library_perm(name, gk))
    info = kept.graph_retained()
    assert info["state"] == 1 and info["builds"] == 1 and info["selected_inverses"] == 0 and info["served"] == 0
    want = as_bytes(ask(plain, gk))
    assert as_bytes(ask(kept, gk)) == want and as_bytes(ask(kept, gk)) == want
    pairs, frm, to, query = K.requests(gk)
    info = kept.graph_retained()
    print(f"{name}: {info}")
    # one build, one selected inverse for six calls; the newest frame's column is solved by the first gate and serves the candidates and
    # every later call (the gate's other `to` frame costs a column per call, where its pairs lie outside the envelope)
    assert info["builds"] == 1 and info["extensions"] == 0 and info["selected_inverses"] == (1 if info["n_free"] else 0) and info["served"] == 6
    assert plain.graph_retained()["state"] == 0
    before = info["columns"]
    got = kept.graph_loop_candidates(query, K.CAND["min_gap"], K.CAND["radius"], K.CAND["k_sigma"], gk["fixed"], capacity=512)
    gate = kept.graph_edge_gate(frm[to == query], to[to == query], None, None, gk["fixed"])
    assert kept.graph_retained()["columns"] == before                  # the column of `query` is there: candidates, then gates into it
    assert as_bytes((np.zeros(0), gate, got)) == as_bytes((np.zeros(0), plain.graph_edge_gate(frm[to == query], to[to == query], None, None, gk["fixed"]),
                                                            plain.graph_loop_candidates(query, K.CAND["min_gap"], K.CAND["radius"], K.CAND["k_sigma"], gk["fixed"], capacity=512)))
    kept.graph_release()
    assert kept.graph_retained()["state"] == 0 and as_bytes(ask(kept, gk)) == want
    kept.close()
    plain.close()


def held(name, gk, poses, got, label):
    """(c): the answers against the restatement, each in its unit"""
    pairs, frm, to, query = K.requests(gk)
    cov, gate, cand, S, prob = K.restated(name, gk, poses)
    cs = K.cov_spread(cov, got[0], pairs, S, prob)
    gs = K.gate_spread(gate, got[1], frm, to, gk["fixed"])
    scale = max(1.0, max(float(np.max(np.abs(p))) for p in poses.values()))
    rel = float(np.max(np.abs(gate[0] - got[1][0]))) / scale
    r = float(np.max(np.abs(gate[1] - got[1][1]))) / scale
    print(f"{name} ({label}): {len(pairs)} blocks {cs:.2e} (tolerance {TOL[name + '/cov']:.2e}); {len(frm)} pairs: S {gs:.2e}, rel {rel:.2e}, r {r:.2e} (tolerance {TOL[name]:.2e})")
    assert cs <= TOL[name + "/cov"] and gs <= TOL[name] and rel <= TOL[name] and r <= TOL[name]
    for p, (a, b) in enumerate(zip(frm.tolist(), to.tolist())):        # chi2 of an r of rounding size has no digits: r^T S^-1 r of what was returned
        if not (a in gk["fixed"] and b in gk["fixed"]):
            mine = float(got[1][1][p] @ np.linalg.solve(got[1][2][p], got[1][1][p]))
            assert got[1][3][p] >= 0.0 and abs(got[1][3][p] - mine) <= 100.0 * np.finfo(float).eps * np.linalg.cond(got[1][2][p]) * max(mine, 1e-300)
    if name == "lap454_open":                                          # the candidate lists
        frames, dist, sigma, margin = cand
        assert margin.min() > 1e-6
        want = dist <= K.CAND["radius"] + K.CAND["k_sigma"] * sigma
        assert got[2][0].tolist() == frames[want].tolist()
        assert np.max(np.abs(got[2][1] - dist[want])) <= TOL[name] * scale and np.max(np.abs(got[2][2] - sigma[want]) / sigma[want]) <= TOL[name]


@pytest.mark.parametrize("name", K.GROWN)
def test_b_c_an_extension_equals_a_rebuild_to_the_bit(name):
    g, st = K.stages(name)
    grown = api.Context(0)
    grown.graph_reset(g.get("edge_capacity", 0))
    append(grown, g, st[0])
    grown.graph_retain(g["fixed"])
    rule = rule_through_stages(name)                                   # the host function's word on every stage: a rebuild where it says so
    whole = api.Context(0)                                             # loads every state at once and retains in the grown context's order
    numpy_held = K.held_states(name)
    last, partial, rebuilds = None, 0, 0
    for k in range(len(st)):
        if k:
            append(grown, g, st[k])
            assert grown.graph_retained()["state"] == 2
        gk = K.state(name, k)
        last = ask(grown, gk)
        info = grown.graph_retained()
        rebuilds += k > 0 and rule[k]["rebuilt"]
        assert info["state"] == 1 and info["extensions"] == k and info["rebuilds"] == rebuilds and info["builds"] == 1, (k, info)
        if k:                                                          # (an edge to a fixed frame can dirty an earlier row than the rule's)
            assert 0 < info["rows_refactored"] and info["first_dirty_row"] + info["rows_refactored"] == info["n_free"], (k, info)
            assert info["first_dirty_row"] <= rule[k]["first_dirty_row"] and info["work"] == rule[k]["work"], (k, info, rule[k])
            partial += info["rows_refactored"] < info["n_free"]
        if k in numpy_held:
            held(name, gk, poses_of(grown, gk), last, f"stage {k}")
        load(whole, gk)                                                # EVERY state: the extended factor's answers are a full factorisation's, to the bit
        whole.graph_retain(g["fixed"], perm=info["perm"])
        assert as_bytes(ask(whole, gk)) == as_bytes(last), k
        wi = whole.graph_retained()
        assert wi["builds"] == 1 and wi["extensions"] == 0 and (wi["widest_row"], wi["blocks"], wi["work"]) == (info["widest_row"], info["blocks"], info["work"])
    info = grown.graph_retained()
    # every extension refactors fewer rows than there are, but chain5's first (frame 3 has an edge to frame 1, which is row 0) and the
    # rebuilds the rule asks for (chain250_split's loop edge and the two appends behind it)
    assert partial == len(st) - 1 - rebuilds - (name == "chain5") and rebuilds == (3 if name == "chain250_split" else 0)
    print(f"{name}: {len(st) - 1} extensions, the last from row {info['first_dirty_row']} of {info['n_free']}; work {info['work']}")
    gk = K.final(name)
    assert state_bytes(whole, gk) == state_bytes(grown, gk)
    grown.close()
    whole.close()


def test_d_closing_the_ring_extends_then_rebuilds():
    """ring70_open's held closing edge is (69, 0) and frame 0 is FIXED: it joins no two free nodes, so the order's rule sees no new edge
    and the extension refactors the one row of frame 69 -- not a rebuild, as the feature's plan expected of it.  What does force one on
    this graph: the ring's other closing edges, between the free frames 67 .. 69 and 1 .. 3 (no single held outlier does: with a chord
    velo_graph_order's own order costs more than the frame order's 2 x)."""
    name = "ring70_open"
    g, st = K.stages(name)
    ctx = api.Context(0)
    load(ctx, K.final(name))
    ctx.graph_retain(g["fixed"])
    assert ctx.graph_retained()["perm"].tolist() == list(range(69))   # frame order
    true = g["held"][g["true_held"][0]]
    assert (true[0], true[1]) == (69, 0)
    ctx.graph_add_edges_weighted([true[0]], [true[1]], [true[2]], np.array([true[3]]), [0.0])
    gk = dict(K.final(name))
    gk["edges"] = gk["edges"] + [(true[0], true[1], true[2], true[3], 0.0)]
    got = ask(ctx, gk)
    info = ctx.graph_retained()
    assert info["state"] == 1 and info["extensions"] == 1 and info["rebuilds"] == 0 and info["first_dirty_row"] == 68 and info["rows_refactored"] == 1, info
    held(name, gk, poses_of(ctx, gk), got, "closed at the fixed frame")
    wrap = [(69, 1), (68, 1), (69, 2), (67, 1), (68, 2), (69, 3)]
    more = [(a, b, Q.relative(g["poses"][a], g["poses"][b]), g["edges"][0][3], 0.0) for a, b in wrap]
    add_edges(ctx, more)
    gk["edges"] = gk["edges"] + more
    got = ask(ctx, gk)
    info = ctx.graph_retained()
    assert info["state"] == 1 and info["extensions"] == 2 and info["rebuilds"] == 1 and info["first_dirty_row"] == 0 and info["rows_refactored"] == 69, info
    assert info["perm"].tolist() != list(range(69))
    held(name, gk, poses_of(ctx, gk), got, "closed between free frames: rebuilt")
    whole = api.Context(0)                                             # and the rebuilt factor is a fresh one's, to the bit
    load(whole, gk)
    whole.graph_retain(g["fixed"], perm=info["perm"])
    assert as_bytes(ask(whole, gk)) == as_bytes(got)
    whole.close()
    ctx.close()
    # the held edges at the optimum of the open graph, through a retained state: as test_gpu_pose_graph_gate.py records them
    from test_gpu_pose_graph_gate import compare, sigma_at
    from test_gpu_pose_graph_gate import TOL as GATE_TOL
    ctx = api.Context(0)
    g2, prob = Q.fixture(name)
    load(ctx, g2)
    ctx.graph_optimize(g2["fixed"], linear_solver="envelope")
    ctx.graph_retain(g2["fixed"])
    poses = poses_of(ctx, g2)
    at, S = sigma_at(g2, prob, poses)
    frm, to = np.array([e[0] for e in g2["held"]], np.int32), np.array([e[1] for e in g2["held"]], np.int32)
    z, info21 = np.array([e[2] for e in g2["held"]]), np.array([e[3] for e in g2["held"]])
    got = ctx.graph_edge_gate(frm, to, z, info21, g2["fixed"])
    assert ctx.graph_retained()["served"] == 1 and GATE_TOL[name] == 100.0 * 9.1e-14
    compare(name, "held, optimised, retained", got, Q.gate(S, at, poses, frm, to, z, info21), poses, frm, to, g2["fixed"], "ring70_open/chi2")
    is_true = np.array([k in g2["true_held"] for k in range(len(frm))])
    assert np.all(got[3][is_true] < 30.0) and np.all(got[3][~is_true] > 300.0)
    ctx.close()


def test_e_what_drops_the_state():
    name = "chain5"
    gk = K.final(name)
    plain = api.Context(0)
    load(plain, gk)
    want = as_bytes(ask(plain, gk))
    ctx = api.Context(0)

    def fresh():
        load(ctx, gk)
        ctx.graph_retain(gk["fixed"])
        assert ctx.graph_retained()["state"] == 1

    fresh()                                                            # another fixed set: served un-retained, the state stays
    other = ctx.graph_covariance([1, 2], [0, 4])
    assert other.tobytes() == plain.graph_covariance([1, 2], [0, 4]).tobytes()
    info = ctx.graph_retained()
    assert info["state"] == 1 and info["served"] == 0
    ctx.graph_set_pose(2, gk["poses"][2])                              # a frame that has a pose, even to the same pose
    assert ctx.graph_retained()["state"] == 0 and as_bytes(ask(ctx, gk)) == want
    fresh()
    ctx.graph_optimize(gk["fixed"])
    assert ctx.graph_retained()["state"] == 0
    plain.graph_optimize(gk["fixed"])
    assert as_bytes(ask(ctx, gk)) == as_bytes(ask(plain, gk))
    fresh()
    ctx.graph_reset()
    assert ctx.graph_retained()["state"] == 0
    fresh()                                                            # the first weighted edge promotes the store
    e = gk["edges"][0]
    ctx.graph_add_edges_weighted([e[0]], [e[1]], [e[2]], np.array([np.eye(6)]), [0.0])
    assert ctx.graph_retained()["state"] == 0
    load(plain, gk)
    plain.graph_add_edges_weighted([e[0]], [e[1]], [e[2]], np.array([np.eye(6)]), [0.0])
    assert as_bytes(ask(ctx, gk)) == as_bytes(ask(plain, gk))
    sparse = dict(gk, poses={f: p for f, p in gk["poses"].items() if f != 1}, edges=[e for e in gk["edges"] if 1 not in e[:2]])
    load(ctx, sparse)                                                  # a posed frame numbered below a retained free one
    ctx.graph_retain(gk["fixed"])
    ctx.graph_set_pose(1, gk["poses"][1])
    assert ctx.graph_retained()["state"] == 0
    late = [e for e in gk["edges"] if 1 in e[:2]]                      # frame 1 took free index 0 and moved every other one: the bytes are a fresh context's
    add_edges(ctx, late)
    assert ctx.graph_retained()["state"] == 0
    load(plain, sparse)
    plain.graph_set_pose(1, gk["poses"][1])
    add_edges(plain, late)
    after = dict(gk, edges=sparse["edges"] + late)
    got = as_bytes(ask(ctx, after))
    assert got == as_bytes(ask(plain, after)) and ctx.graph_retained()["served"] == 0
    ctx.close()
    plain.close()


def test_f_a_new_frame_without_an_edge_is_refused_and_the_state_stays_behind():
    name = "chain5"
    g, st = K.stages(name)
    ctx, plain, whole = api.Context(0), api.Context(0), api.Context(0)
    for c in (ctx, plain):
        c.graph_reset()
        append(c, g, st[0])
    ctx.graph_retain(g["fixed"])
    before = ctx.graph_retained()
    for c in (ctx, plain):
        c.graph_set_pose(3, g["poses"][3])
    errors = []
    for c in (ctx, plain):
        with pytest.raises(api.VeloError, match="status -1.*velo_graph_covariance.*not positive definite.*frame 3") as err:
            c.graph_covariance([1, 3], g["fixed"])
        errors.append(str(err.value))
    assert errors[0] == errors[1]
    after = ctx.graph_retained()
    assert after["state"] == 2 and after["n_free"] == before["n_free"] == 2 and after["extensions"] == 0 and after["perm"].tolist() == before["perm"].tolist()
    add_edges(ctx, st[1][1])
    gk = K.state(name, 1)
    got = ask(ctx, gk)
    info = ctx.graph_retained()
    assert info["state"] == 1 and info["extensions"] == 1 and info["n_free"] == 3
    load(whole, gk)
    whole.graph_retain(g["fixed"], perm=info["perm"])
    assert as_bytes(ask(whole, gk)) == as_bytes(got)
    for c in (ctx, plain, whole):
        c.close()


def test_g_asking_changes_nothing_a_solve_sees():
    name = "ring70_open"
    g, st = K.stages(name)
    gk = K.final(name)
    asked, plain = api.Context(0), api.Context(0)
    asked.graph_reset()
    append(asked, g, st[0])
    asked.graph_retain(g["fixed"])
    for k in range(1, len(st)):
        append(asked, g, st[k])
        if k % 10 == 0:
            ask(asked, K.state(name, k))
    first = as_bytes(ask(asked, gk))
    again = api.Context(0)                                             # the same calls, the same bytes
    again.graph_reset()
    append(again, g, st[0])
    again.graph_retain(g["fixed"])
    for k in range(1, len(st)):
        append(again, g, st[k])
        if k % 10 == 0:
            ask(again, K.state(name, k))
    assert as_bytes(ask(again, gk)) == first
    again.close()
    load(plain, gk)
    assert state_bytes(asked, gk) == state_bytes(plain, gk) and asked.graph_info() == plain.graph_info()
    with pytest.raises(api.VeloError, match="status -1.*velo_graph_retain.*not a permutation"):
        asked.graph_retain(g["fixed"], perm=[0] * 69)
    with pytest.raises(api.VeloError, match="status -1.*velo_graph_retain.*over the cap of 1 "):
        asked.graph_retain(g["fixed"], max_work=1)
    assert asked.graph_retained()["state"] == 1 and as_bytes(ask(asked, gk)) == first      # a refusal leaves the state alone
    asked.graph_release()
    out = []
    for ctx in (asked, plain):
        for solver in ("envelope", "cg"):
            s = ctx.graph_optimize(g["fixed"], linear_solver=solver)
            out.append(summary_bytes(s) + state_bytes(ctx, gk))
            if ctx is asked:
                ctx.graph_retain(g["fixed"])
                ask(ctx, gk)
    assert out[:2] == out[2:] and asked.graph_info() == plain.graph_info()
    asked.close()
    plain.close()


def test_h_queries_of_every_kind_in_any_order_share_the_buffers():
    """The tests above ask covariance, gate, candidates, always in that order.  Here a retained and a never-retaining context are asked
    gate, candidates, covariance, candidates without sigma, a gate of three columns (the column buffer grows, the kept column survives),
    the first gate again: sizes shrink and grow between kinds, and every answer is a fresh never-retaining context's asked that alone."""
    gk = K.final("ring70_open")
    fx = gk["fixed"]
    pairs, frm, to, query = K.requests(gk)
    far_from, far_to = np.array([5, 60, 10], np.int32), np.array([query, 20, 50], np.int32)     # three distinct free `to` frames, each pair 40 and more apart
    questions = [lambda c: c.graph_edge_gate(frm, to, None, None, fx),
                 lambda c: c.graph_loop_candidates(query, K.CAND["min_gap"], K.CAND["radius"], K.CAND["k_sigma"], fx, capacity=512),
                 lambda c: (c.graph_covariance(pairs, fx),),
                 lambda c: c.graph_loop_candidates(query, K.CAND["min_gap"], K.CAND["radius"], 0.0, fx, capacity=512),
                 lambda c: c.graph_edge_gate(far_from, far_to, None, None, fx),
                 lambda c: c.graph_edge_gate(frm, to, None, None, fx)]
    as_b = lambda ans: b"".join(np.asarray(x).tobytes() for x in ans)  # noqa: E731
    want = []
    for q in questions:
        alone = api.Context(0)
        load(alone, gk)
        want.append(as_b(q(alone)))
        alone.close()
    kept, never = api.Context(0), api.Context(0)
    load(kept, gk)
    load(never, gk)
    kept.graph_retain(fx, perm=library_perm("ring70_open", gk))       # (a): the bytes are an un-retained context's in the library's own order
    columns = [0]
    for k, q in enumerate(questions):
        assert as_b(q(never)) == want[k], k
        assert as_b(q(kept)) == want[k], k
        columns.append(kept.graph_retained()["columns"])
    solved = np.diff(columns).tolist()
    info = kept.graph_retained()
    print(f"ring70_open: full columns solved per question {solved}; {info}")
    # the precondition, from the state's own counters: the three-column gate keeps the query's column (the candidates' before it) and solves two,
    # the first gate asked again keeps it too and solves the other `to` frame's: columns were solved and columns were reused
    needed = [len(set(to.tolist())), 1, 0, 0, 3, len(set(to.tolist()))]
    reused = [n - s for n, s in zip(needed, solved)]
    assert solved[4] == 2 and reused[4] == 1 and solved[5] >= 1 and reused[5] >= 1, (solved, needed)
    assert info["state"] == 1 and info["served"] == 5 and info["selected_inverses"] == 1 and info["builds"] == 1 and never.graph_retained()["state"] == 0
    kept.close()
    never.close()
