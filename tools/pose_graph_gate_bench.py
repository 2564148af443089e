#!/usr/bin/env python3
"""The edge gate and the loop candidates on a drive's pose graph: host times on the synthetic drive of
tools/pose_graph_bench.py (4,541 poses, odometry for dframe 1 .. 4 and the reference's loop edges), after one envelope solve:

  candidates             one velo_graph_loop_candidates call for the last frame with k_sigma 3 (factorisation, selected inverse, ONE full
                         column, a thread per frame), and with k_sigma 0 (no factorisation)
  gate, 32 against one   one velo_graph_edge_gate call for 32 frames spread over the drive against the last frame: one full column
  covariance, 96 blocks  what a caller had before: velo_graph_covariance for the three blocks of each of those 32 pairs, 32 column solves;
                         interleaved with the line above, repetition by repetition
  full column / pair column   a gate of one pair outside the envelope minus a gate of one pair inside it, and the same difference for
                         velo_graph_covariance: the two column kernels per launch
  optimize, covariance   the envelope solve and the all-marginals call of tools/pose_graph_cov_bench.py in the same run

Every call ends in a device synchronisation; the host clock is around the Python call.  A launch alone is a kernel trace's to give: run
this tool under `rocprofv3 --kernel-trace --stats`, a run of its own.  Nothing gates on this tool.
Usage: python tools/pose_graph_gate_bench.py [--reps 5] [--out profiles/r26_pose_graph_gate.txt]"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import velo_amd  # noqa: E402,F401
import pose_graph_bench as B  # noqa: E402
import pose_graph_gate_ref as Q  # noqa: E402
import pose_graph_ref as G  # noqa: E402


LOOP_RADIUS = B.LOOP_CLOSE_THRESH


def once(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def interleaved(fns, reps):
    """every function once per repetition, in turn, after one warm-up round (the buffers are allocated in it)"""
    ms, out = [[] for _ in fns], [None] * len(fns)
    for rep in range(reps + 1):
        for k, fn in enumerate(fns):
            t, out[k] = once(fn)
            if rep > 0:
                ms[k].append(t)
    return ms, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from velo_amd import api
    g = B.make_drive()
    N = B.N
    start = np.array([g["poses"][i] for i in range(N)])
    frm, to = [e[0] for e in g["edges"]], [e[1] for e in g["edges"]]
    z, info = np.array([e[2] for e in g["edges"]]), [e[3] for e in g["edges"]]
    prob = G.problem_of(g)
    pairs = [(prob.slot[e[0]], prob.slot[e[1]]) for e in g["edges"] if e[0] in prob.slot and e[1] in prob.slot]
    perm, first, stats = api.graph_order(prob.n_free, [p[0] for p in pairs], [p[1] for p in pairs])
    pos = np.empty(prob.n_free, dtype=np.int64)
    pos[np.asarray(perm, dtype=np.int64)] = np.arange(prob.n_free)
    query = N - 1
    outside = lambda f: first[max(pos[prob.slot[f]], pos[prob.slot[query]])] > min(pos[prob.slot[f]], pos[prob.slot[query]])   # noqa: E731
    cand = [int(f) for f in np.linspace(1, N - 200, 400).astype(int) if outside(int(f))]
    cand = [cand[k] for k in np.linspace(0, len(cand) - 1, 32).astype(int)]
    assert len(set(cand)) == 32
    gate_frm, gate_to = np.asarray(cand, np.int32), np.full(32, query, np.int32)
    blocks = np.array([q for f in cand for q in ((f, f), (f, query), (query, query))], dtype=np.int32)
    inside = (query - 1, query)
    ctx = api.Context(0)
    ctx.graph_reset(len(frm))
    ctx.graph_set_poses(0, start)
    ctx.graph_add_edges(frm, to, z, info)
    ctx.synchronize()
    t_opt, s = once(lambda: ctx.graph_optimize(g["fixed"], linear_solver="envelope"))
    fx = g["fixed"]
    (ms_gate, ms_cov96), (gate, cov96) = interleaved([lambda: ctx.graph_edge_gate(gate_frm, gate_to, None, None, fx), lambda: ctx.graph_covariance(blocks, fx)], a.reps)
    (ms_k3, ms_k0), (c3, c0) = interleaved([lambda: ctx.graph_loop_candidates(query, 50, LOOP_RADIUS, 3.0, fx, capacity=N), lambda: ctx.graph_loop_candidates(query, 50, LOOP_RADIUS, 0.0, fx, capacity=N)], a.reps)
    (ms_g_out, ms_g_in, ms_c_out, ms_c_in), _ = interleaved([lambda: ctx.graph_edge_gate([cand[0]], [query], None, None, fx), lambda: ctx.graph_edge_gate([inside[0]], [inside[1]], None, None, fx),
                                                             lambda: ctx.graph_covariance([(cand[0], query)], fx), lambda: ctx.graph_covariance([inside], fx)], a.reps)
    (ms_all,), _ = interleaved([lambda: ctx.graph_covariance(np.arange(N), fx)], a.reps)
    poses = {f: p for f, p in enumerate(ctx.graph_get_poses(0, N))}
    ctx.close()
    # the gate's S against the same formula on the covariance call's blocks, in numpy: the two paths agree
    worst = 0.0
    for k, f in enumerate(cand):
        _, _, _, A, Bm = Q.pair_terms(poses, f, query)
        Saa, Sab, Sbb = cov96[3 * k], cov96[3 * k + 1], cov96[3 * k + 2]
        worst = max(worst, Q.rel_spread(A @ Saa @ A.T + A @ Sab @ Bm.T + Bm @ Sab.T @ A.T + Bm @ Sbb @ Bm.T, gate[2][k]))
    lines = [f"pose graph: {N} poses, {g['n_odometry']} odometry edges (dframe 1..4), {len(g['edges']) - g['n_odometry']} loop edges; {prob.n_free} free nodes, "
             f"widest row {stats['widest_row']} blocks, envelope {stats['envelope_blocks']} blocks, work {stats['work']} block products per factorisation",
             f"GPU  envelope solver: optimize {t_opt:.2f} ms, {s.iterations} LM iterations ({t_opt / max(s.iterations, 1):.2f} ms each), termination {s.termination}, "
             f"cost {s.initial_cost:.4e} -> {s.final_cost:.4e}",
             f"GPU  covariance, all {N} marginals in one call: {B.med(ms_all)} ms",
             f"GPU  loop candidates of frame {query} (min_gap 50, radius {LOOP_RADIUS} m), k_sigma 3: {B.med(ms_k3)} ms, {len(c3[0])} frames; k_sigma 0 (no factorisation): {B.med(ms_k0)} ms, {len(c0[0])} frames",
             f"GPU  edge gate, 32 frames against frame {query}, all outside the envelope, ONE full column: {B.med(ms_gate)} ms",
             f"GPU  covariance, the 96 blocks of the same 32 pairs, 32 column solves (interleaved with the line above): {B.med(ms_cov96)} ms",
             f"GPU  edge gate, one pair outside the envelope {B.med(ms_g_out)} ms, one pair inside {B.med(ms_g_in)} ms: the full column is the difference, {np.median(ms_g_out) - np.median(ms_g_in):.2f} ms",
             f"GPU  covariance, one pair outside the envelope {B.med(ms_c_out)} ms, one pair inside {B.med(ms_c_in)} ms: the pair column is the difference, {np.median(ms_c_out) - np.median(ms_c_in):.2f} ms",
             f"largest sigma of a candidate's relative position {c3[2].max() if len(c3[2]) else 0.0:.3f} m; chi2 of the 32 stored relative poses against themselves at most {gate[3].max():.2e}; "
             f"the gate's 32 S against A S A^T of the covariance call's 96 blocks in numpy: {worst:.2e} sigma_i sigma_j"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
