"""Dev tool: the pose graph's queries on ring70_open in a fixed sequence, for comparing what two builds enqueue.  On the library of the tree
given as argv[1] (this tree: `.`; another checkout built beside it: its root): per-call covariance / gate / candidates, velo_graph_retain, the
three queries twice, one stage appended, the three queries.  Prints a SHA-256 of every step's answers.

    rocprofv3 --kernel-trace --memory-copy-trace --output-format csv json -d OUT_A -- python tools/pose_graph_launch_seq.py TREE_A
    (the same for TREE_B, a run of its own), then  python tools/pose_graph_launch_diff.py OUT_A OUT_B     (profiles/r28_pose_graph_queries.txt)"""
import hashlib
import os
import sys

ROOT = os.path.abspath(sys.argv[1])
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402
import velo_amd  # noqa: E402,F401
import pose_graph_retained_cases as K  # noqa: E402
from velo_amd import api  # noqa: E402

assert os.path.abspath(api.__file__).startswith(os.path.join(ROOT, "vision-enhanced-lidar-odometry_amd") + os.sep), api.__file__
print("library", api.load_library()._name, flush=True)


def add_edges(ctx, edges):
    for e in edges:                                                    # one call per edge: the kind of each decides the entry
        if np.ndim(e[3]) == 0:
            ctx.graph_add_edges([e[0]], [e[1]], [e[2]], [e[3]])
        else:
            ctx.graph_add_edges_weighted([e[0]], [e[1]], [e[2]], np.array([e[3]]), [e[4]])


def ask(ctx, gk, label):
    pairs, frm, to, query = K.requests(gk)
    out = [ctx.graph_covariance(pairs, gk["fixed"])]
    out += list(ctx.graph_edge_gate(frm, to, None, None, gk["fixed"]))
    out += list(ctx.graph_loop_candidates(query, K.CAND["min_gap"], K.CAND["radius"], K.CAND["k_sigma"], gk["fixed"], capacity=512))
    print(label, hashlib.sha256(b"".join(np.asarray(x).tobytes() for x in out)).hexdigest(), flush=True)


name = "ring70_open"
g, st = K.stages(name)
k = len(st) - 2
gk = K.state(name, k)
ctx = api.Context(0)
ctx.graph_reset(g.get("edge_capacity", 0))
for f in sorted(gk["poses"]):
    ctx.graph_set_pose(f, gk["poses"][f])
add_edges(ctx, gk["edges"])
ask(ctx, gk, "per-call")
ctx.graph_retain(g["fixed"])
ask(ctx, gk, "retained 1")
ask(ctx, gk, "retained 2")
frames, edges = st[k + 1]
for f in frames:
    ctx.graph_set_pose(f, g["poses"][f])
add_edges(ctx, edges)
ask(ctx, K.state(name, k + 1), "appended")
info = ctx.graph_retained()
print("info", {a: b for a, b in info.items() if a != "perm"}, flush=True)
ctx.close()
