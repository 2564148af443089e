#!/usr/bin/env python3
"""The retained factorisation on a drive's pose graph: host times on the synthetic drive of tools/pose_graph_bench.py
(4,541 poses, odometry for dframe 1 .. 4 and the reference's loop edges), after one envelope solve and velo_graph_retain, against the
same calls on a second context that retains nothing, in the same process, interleaved:

  per appended frame     a node with its dead-reckoned pose and one odometry edge, then one velo_graph_loop_candidates call (k_sigma 3) for the
                         new frame -- on the retained context the call that extends the state -- and one 32-pair velo_graph_edge_gate against it
  a current state        the same two calls again, nothing appended in between: no factorisation, no selected inverse, the column kept
  an extension alone     append, then velo_graph_retain: the order's rule, the system, the rows from the first dirty one on
  a loop edge            an edge from the newest frame to a frame far back, then velo_graph_retain: what the order's rule decides and costs
  the newest frame       where velo_graph_order puts it, and where velo_graph_order_extend's orientation does
  the first append       after velo_graph_retain, and again after the rebuild: the state is in velo_graph_order's (oriented) order, in which the newest
                         frame does NOT sit at the end, so the first append dirties from that frame's row on; the appends behind it from the end
  --hash                 SHA-256 of velo_graph_optimize's summary and poses, of all marginals, of the 96-block covariance call, of one 32-pair gate
                         and one k_sigma 3 candidates call before anything is retained; of that gate and those candidates asked twice once
                         the state is retained, and of velo_graph_retained's info after them; and nothing else
  --parent-record FILE   the --hash --out FILE lines of the PARENT commit's library, to be stated beside this library's and compared.  The parent's
                         tree has no such tool: check the parent commit out beside this tree, build it, copy this file into its tools/ and run it
                         there with --hash --out FILE (it imports the tree it lies in; --hash uses no entry the parent lacks)

Every call ends in a device synchronisation; the host clock is around the Python call.  Nothing gates on this tool.
Usage: python tools/pose_graph_retained_bench.py [--reps 3] [--hash] [--parent-record FILE] [--out profiles/r27_pose_graph_retained.txt]"""
import argparse
import ctypes as C
import hashlib
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


def once(fn):
    t0 = time.perf_counter()
    out = fn()
    return 1e3 * (time.perf_counter() - t0), out


def load(api, g):
    N = B.N
    ctx = api.Context(0)
    ctx.graph_reset(len(g["edges"]) + 64)
    ctx.graph_set_poses(0, np.array([g["poses"][i] for i in range(N)]))
    ctx.graph_add_edges([e[0] for e in g["edges"]], [e[1] for e in g["edges"]], np.array([e[2] for e in g["edges"]]), [e[3] for e in g["edges"]])
    return ctx


def gate_frames(query):
    return np.linspace(1, query - 200, 32).astype(np.int32), np.full(32, query, np.int32)


def hashes(api, g):
    """the un-retained bytes of optimize, all marginals, the 96 blocks of 32 pairs against the last frame, their gate and the last frame's
    candidates; the gate's and the candidates' again, twice, once that state is retained, and velo_graph_retained's info after them"""
    N = B.N
    ctx = load(api, g)
    s = ctx.graph_optimize(g["fixed"], linear_solver="envelope")
    poses = ctx.graph_get_poses(0, N)
    marg = ctx.graph_covariance(np.arange(N), g["fixed"])
    frm, to = gate_frames(N - 1)
    blocks = np.array([q for f in frm for q in ((f, f), (f, N - 1), (N - 1, N - 1))], dtype=np.int32)
    cov96 = ctx.graph_covariance(blocks, g["fixed"])
    sha = lambda b: hashlib.sha256(b).hexdigest()                      # noqa: E731
    ans = lambda x: b"".join(np.asarray(v).tobytes() for v in x)       # noqa: E731
    gate = lambda c: ans(c.graph_edge_gate(frm, to, None, None, g["fixed"]))                                                  # noqa: E731
    cand = lambda c: ans(c.graph_loop_candidates(N - 1, 50, B.LOOP_CLOSE_THRESH, 3.0, g["fixed"], capacity=N + 64))           # noqa: E731
    out = [f"sha256 optimize (summary, poses)  {sha(C.string_at(C.addressof(s), C.sizeof(s)) + poses.tobytes())}",
           f"sha256 covariance, {N} marginals   {sha(marg.tobytes())}", f"sha256 covariance, 96 blocks        {sha(cov96.tobytes())}",
           f"sha256 gate, 32 pairs, un-retained   {sha(gate(ctx))}", f"sha256 candidates, un-retained      {sha(cand(ctx))}"]
    ctx.graph_retain(g["fixed"])                                       # the same state retained, each asked twice, and what the state counts
    out += [f"sha256 {what}, retained, {nth}   {sha(fn(ctx))}" for nth in ("1st", "2nd") for what, fn in (("gate, 32 pairs", gate), ("candidates", cand))]
    info = ctx.graph_retained()
    out.append("sha256 velo_graph_retained's info    " + sha(repr(sorted((k, np.asarray(v).tolist()) for k, v in info.items())).encode()))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--hash", action="store_true")
    ap.add_argument("--parent-record", default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from velo_amd import api
    g = B.make_drive()
    N, fx = B.N, g["fixed"]
    lines = hashes(api, g)
    if a.parent_record:
        with open(a.parent_record) as f:
            parent = [line.rstrip("\n") for line in f if line.startswith("sha256 ")]
        same = parent == lines
        lines += ["parent  " + line for line in parent]
        lines.append("the parent commit's library, a process of its own: " + (f"the SAME {len(parent)} digests" if same else "DIFFERENT digests"))
    if not a.hash:
        kept, plain = load(api, g), load(api, g)
        for ctx in (kept, plain):
            ctx.graph_optimize(fx, linear_solver="envelope")
        t_retain, _ = once(lambda: kept.graph_retain(fx))
        built = kept.graph_retained()
        pairs = [(e[0] - 1, e[1] - 1) for e in g["edges"] if e[0] > 0 and e[1] > 0]
        perm, first, stats = api.graph_order(N - 1, [p[0] for p in pairs], [p[1] for p in pairs])
        _, _, oriented = api.graph_order_extend(0, [], N - 1, [p[0] for p in pairs], [p[1] for p in pairs], 0, 0)
        at = int(np.nonzero(perm == N - 2)[0][0])
        lines += [f"pose graph: {N} poses, {g['n_odometry']} odometry edges (dframe 1..4), {len(g['edges']) - g['n_odometry']} loop edges; velo_graph_order: widest row "
                  f"{stats['widest_row']}, work {stats['work']}; the newest frame at position {at} of {N - 1}; velo_graph_order_extend's orientation "
                  f"{'reverses it: position ' + str(N - 2 - at) if oriented['reversed'] else 'leaves it'} (work {oriented['fresh_work']})",
                  f"GPU  velo_graph_retain after the solve: {t_retain:.2f} ms; the order {'rebuilt (velo_graph_order, oriented)' if built['perm'].tolist() != list(range(N - 1)) else 'in frame order'}, "
                  f"widest row {built['widest_row']}, work {built['work']}"]
        z_odo = g["edges"][N - 2][2]                                   # the last dframe-1 measurement: the dead-reckoned step
        rows = dict(kc=[], kg=[], pc=[], pg=[], kc2=[], kg2=[], p=[], rr=[], rb=[])
        newest = N - 1
        for rep in range(a.reps + 1):
            pose = G.compose(kept.graph_get_poses(newest, 1)[0], z_odo)
            newest += 1
            for ctx in (kept, plain):
                ctx.graph_set_pose(newest, pose)
                ctx.graph_add_edges([newest - 1], [newest], [z_odo], [1.0])
            frm, to = gate_frames(newest)
            t = [once(lambda c=c: c.graph_loop_candidates(newest, 50, B.LOOP_CLOSE_THRESH, 3.0, fx, capacity=N + 64))[0] for c in (kept, plain)]
            info = kept.graph_retained()
            t += [once(lambda c=c: c.graph_edge_gate(frm, to, None, None, fx))[0] for c in (kept, plain)]
            t += [once(lambda: kept.graph_loop_candidates(newest, 50, B.LOOP_CLOSE_THRESH, 3.0, fx, capacity=N + 64))[0], once(lambda: kept.graph_edge_gate(frm, to, None, None, fx))[0]]
            if rep == 0:
                first = (info["first_dirty_row"], info["rows_refactored"], info["n_free"], t[0], t[1])
            if rep > 0:
                for k, v in zip(("kc", "pc", "kg", "pg", "kc2", "kg2"), t):
                    rows[k].append(v)
                rows["p"].append(info["first_dirty_row"]); rows["rr"].append(info["rows_refactored"]); rows["rb"].append(info["rebuilds"])
        lines += [f"GPU  the FIRST append after velo_graph_retain (the repetition the lines below leave out; it also allocates the calls' buffers): from row {first[0]}, "
                  f"{first[1]} rows refactored of {first[2]}; its candidates call {first[3]:.2f} / {first[4]:.2f} ms",
                  f"GPU  per appended frame ({a.reps} after 1), retained / un-retained, interleaved:",
                  f"       candidates of the new frame, k_sigma 3 (the retained call extends the state): {B.med(rows['kc'])} / {B.med(rows['pc'])} ms",
                  f"       edge gate, 32 frames against the new frame (a current state, the column kept): {B.med(rows['kg'])} / {B.med(rows['pg'])} ms",
                  f"       the extensions' first dirty rows {rows['p']}, rows refactored {rows['rr']} of {info['n_free']}; rebuilds so far {rows['rb']}",
                  f"GPU  a current state, the same two calls again: candidates {B.med(rows['kc2'])} ms, gate {B.med(rows['kg2'])} ms"]
        ext = []
        for rep in range(a.reps):
            pose = G.compose(kept.graph_get_poses(newest, 1)[0], z_odo)
            newest += 1
            kept.graph_set_pose(newest, pose)
            kept.graph_add_edges([newest - 1], [newest], [z_odo], [1.0])
            ext.append(once(lambda: kept.graph_retain(fx))[0])
        info = kept.graph_retained()
        lines.append(f"GPU  an extension alone (append, velo_graph_retain): {B.med(ext)} ms; the last from row {info['first_dirty_row']}, {info['rows_refactored']} rows refactored, "
                     f"rebuilds so far {info['rebuilds']}")
        before = info["rebuilds"]
        kept.graph_add_edges([100], [newest], [G.relative(kept.graph_get_poses(100, 1)[0], kept.graph_get_poses(newest, 1)[0])], [1.0])
        t_loop, _ = once(lambda: kept.graph_retain(fx))
        info = kept.graph_retained()
        lines.append(f"GPU  a loop edge (100, {newest}), velo_graph_retain: {t_loop:.2f} ms; {'REBUILT' if info['rebuilds'] > before else 'extended'} from row {info['first_dirty_row']}, "
                     f"widest row {info['widest_row']}, work {info['work']}")
        after, rebuilds = [], info["rebuilds"]
        for rep in range(2):                                           # the appends behind a rebuild: the first from the newest frame's row in the fresh order
            pose = G.compose(kept.graph_get_poses(newest, 1)[0], z_odo)
            newest += 1
            kept.graph_set_pose(newest, pose)
            kept.graph_add_edges([newest - 1], [newest], [z_odo], [1.0])
            ms = once(lambda: kept.graph_retain(fx))[0]
            info = kept.graph_retained()
            after.append(f"{ms:.2f} ms from row {info['first_dirty_row']}, {info['rows_refactored']} rows of {info['n_free']}" + (" (REBUILT)" if info["rebuilds"] > rebuilds else ""))
            rebuilds = info["rebuilds"]
        lines.append(f"GPU  the two appends after that rebuild (append, velo_graph_retain): {after[0]}; {after[1]}")
        lines.append(f"counters: {({k: v for k, v in info.items() if k != 'perm'})}")
        kept.close()
        plain.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
