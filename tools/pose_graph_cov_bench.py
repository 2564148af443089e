#!/usr/bin/env python3
"""Covariances of a drive's pose graph: the host time of velo_graph_covariance on the synthetic drive of
tools/pose_graph_bench.py (4,541 poses, odometry for dframe 1 .. 4 and the reference's loop edges), after one envelope solve:

  all marginals          one call for the 4,541 marginals: fill, factorisation, selected inverse, gather, one copy
  one pair inside        one call for a single marginal: the same launches, so the gather and the copy are what is saved
  one pair outside       one call for a single pair outside the envelope: the same launches and one column solve; the difference to
                         the line above is the column's time
  optimize, per LM iteration   the envelope solve in the same run: the factorisation beside which the figures above stand

Every call ends in a device synchronisation; the host clock is around the Python call.  The time of a launch alone (the selected
inverse, a column, the factorisation) is a kernel trace's to give: run this tool under `rocprofv3 --kernel-trace --stats`, a run of its
own, and read graph_env_selinv_kernel, graph_env_column_kernel and graph_env_factor_kernel off its table.  Nothing gates on this tool.
Usage: python tools/pose_graph_cov_bench.py [--reps 5] [--out profiles/r24_pose_graph_covariance.txt]"""
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
import pose_graph_ref as G  # noqa: E402


def timed(fn, reps):
    ms, out = [], None
    for rep in range(reps + 1):                                        # one warm-up: the buffers are allocated in it
        t0 = time.perf_counter()
        out = fn()
        if rep > 0:
            ms.append(1e3 * (time.perf_counter() - t0))
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
    hi = max(k for k in range(prob.n_free) if first[k] > 0)           # the last row that leaves columns out, against column 0
    outside = (prob.free[int(perm[hi])], prob.free[int(perm[0])])
    ctx = api.Context(0)
    ctx.graph_reset(len(frm))
    ctx.graph_set_poses(0, start)
    ctx.graph_add_edges(frm, to, z, info)
    ctx.synchronize()
    t0 = time.perf_counter()
    s = ctx.graph_optimize(g["fixed"], linear_solver="envelope")
    t_opt = 1e3 * (time.perf_counter() - t0)
    frames = np.arange(N)
    ms_all, cov = timed(lambda: ctx.graph_covariance(frames, g["fixed"]), a.reps)
    ms_in, one = timed(lambda: ctx.graph_covariance([N - 1], g["fixed"]), a.reps)
    ms_out, cross = timed(lambda: ctx.graph_covariance([outside], g["fixed"]), a.reps)
    ctx.close()
    assert cov[N - 1].tobytes() == one[0].tobytes()
    sig = np.sqrt(np.einsum("kii->ki", cov))
    lines = [f"pose graph: {N} poses, {g['n_odometry']} odometry edges (dframe 1..4), {len(g['edges']) - g['n_odometry']} loop edges; {prob.n_free} free nodes, "
             f"widest row {stats['widest_row']} blocks, envelope {stats['envelope_blocks']} blocks, work {stats['work']} block products per factorisation",
             f"GPU  envelope solver: optimize {t_opt:.2f} ms, {s.iterations} LM iterations ({t_opt / max(s.iterations, 1):.2f} ms each: fill, factorisation, solve, candidate), "
             f"termination {s.termination}, cost {s.initial_cost:.4e} -> {s.final_cost:.4e}",
             f"GPU  covariance, all {N} marginals in one call: {B.med(ms_all)} ms",
             f"GPU  covariance, one marginal (inside the envelope): {B.med(ms_in)} ms",
             f"GPU  covariance, one pair outside the envelope {outside}: {B.med(ms_out)} ms; the column solve is the difference to the line above, "
             f"{np.median(ms_out) - np.median(ms_in):.2f} ms",
             f"largest standard deviation of a position component {sig[:, 3:].max():.3f} m (frame {int(np.argmax(sig[:, 3:].max(axis=1)))}), of a rotation component "
             f"{sig[:, :3].max():.2e} rad; frame 0 (fixed) {sig[0].max():.1f}; largest |cross block| entry of the outside pair {np.abs(cross[0]).max():.3e}"]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
