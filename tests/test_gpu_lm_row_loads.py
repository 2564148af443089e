"""-m gpu: the point-to-plane sweep requests the rows behind its prefetched ones a chunk at a time, addresses clamped at the last query,
and validity predicates the arithmetic only (sweep_rows / row_chunk_request).  Checked at the smallest shapes where such loads can go
wrong, together with the hand-over of a chained call's pose record to the next association round:

  row counts   1, 255, 256, 257, 1023, 1025 and 3 x 256 x 4 + 1 queries at the plan's four rows per thread -- threads that hold no row,
               one, some and all four, the clamp at the last query hit in every one of them;
  more rows    the same 3,073 queries at EIGHT rows per thread (VELO_EVAL_PER_THREAD of the diagnostics build, read once per process:
               a child process): six or seven rows per thread, so the lean kernels take a second chunk (requested inside the loop) and
               the kernels with four prefetched rows take their chunked tail at all -- with a query shard that does not start at 0;
  validity     invalid rows between valid ones: every other row, every row of some threads, every row of a whole workgroup (sources
               moved out of the gate).

What must agree: velo_evaluate / velo_evaluate_rows with the oracle, within the 1e-12 the parity tests use for the sums -- the ROW OUTPUTS
are checked there only, on the sweep kernel of the two-launch path (four prefetched rows); the lean kernels' row-output branch is never
taken by the library.  And -- bit for bit -- the registration of the same pair by the lean sweep + step launches (lock-step group of two
contexts, VELO_LM_LEAN=1), their 126-VGPR form for scan-to-map groups (VELO_LM_SLIM=1), the plain ones (VELO_LM_LEAN=0), the single-pair
one-launch iteration, the one-launch solve and the host-driven two-launch path: pose, every solve's initial and final cost and its
iteration and evaluation counts.  The lean launches expose their 21 + 6 sums and the cost through exactly that: every LM step is a
function of them.  Which kernel a path launched is asserted from the context's launch log.  Nothing here looks at machine code."""
import os
import subprocess
import sys

import numpy as np
import pytest

if __name__ == "__main__":                     # the child process of the last test: the paths and the load order tests/conftest.py sets up
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "tests")]
    import torch  # noqa: F401

import helpers as H
from velo_amd import api, synth

pytestmark = pytest.mark.gpu

ROWS_PER_BLOCK = 256 * 4                       # kEvalThreads x kEvalPerThread (eval_plan)
SIZES = [1, 255, 256, 257, 1023, 1025, 3 * ROWS_PER_BLOCK + 1]
FAR = np.array([0.0, 400.0, 0.0], dtype=np.float32)      # a source moved this far has no target point inside the gate


@pytest.fixture(scope="module")
def pair():
    d = synth.scan_pair(n_beams=16, n_azimuth=300)
    assert len(d["src_xyz"]) >= SIZES[-1]
    return d


def cut(d, n, invalid=None):
    """The pair with the first n source points only (whole rings, then a partial one); invalid: indices of sources moved out of the gate."""
    xyz = np.array(d["src_xyz"][:n], copy=True)
    if invalid is not None:
        xyz[invalid, :3] += FAR
    off = np.unique(np.minimum(np.asarray(d["src_off"]), n)).astype(np.asarray(d["src_off"]).dtype)
    return dict(d, src_xyz=xyz, src_off=off)


def summary_tuple(s):
    return [(s.solves[k].termination, s.solves[k].lm_iterations, s.solves[k].evaluations, s.solves[k].n_icp_valid,
             s.solves[k].initial_cost, s.solves[k].final_cost) for k in range(s.n_solves)]


def load(c, d):
    c.set_target(d["tgt_xyz"], d["tgt_off"])
    c.set_source(d["src_xyz"], d["src_off"])


def check_evaluation(c, orc, d, n_expected=None):
    """cost, the 21 + 6 sums and the rows of the explicit evaluation entry points against the oracle"""
    x = d["x0"]
    nv = c.associate(x, 1)
    assert nv == orc.associate(x, 1)
    H.assert_corr_equal(c.correspondences(), orc.correspondences())
    if n_expected is not None:
        assert nv == n_expected
    c1, H1, g1 = c.evaluate(x)
    c2, H2, g2 = orc.evaluate(x)
    r1, J1 = c.evaluate_rows(x)
    r2, J2 = orc.evaluate_rows(x)
    assert r1.shape == r2.shape == (nv,) and J1.shape == J2.shape
    if nv == 0:
        assert c1 == c2 == 0.0 and not H1.any() and not g1.any()
        return nv
    print(f"n_valid {nv}: cost {abs(c1 - c2) / c2:.1e} H {H.rel_err(H1, H2):.1e} g {H.rel_err(g1, g2):.1e} r {H.rel_err(r1, r2):.1e} J {H.rel_err(J1, J2):.1e}")
    assert abs(c1 - c2) <= 1e-12 * c2 and H.rel_err(H1, H2) <= 1e-12 and H.rel_err(g1, g2) <= 1e-12
    assert H.rel_err(r1, r2) <= 1e-12 and H.rel_err(J1, J2) <= 1e-12
    # the sweep that wrote the rows out left the sums' inputs alone: the same call again gives the same bits
    c3, H3, g3 = c.evaluate(x)
    assert c3 == c1 and np.array_equal(H3, H1) and np.array_equal(g3, g1)
    return nv


# (name, environment of the diagnostics build, contexts in the call, the LM kernel the launch log must name -- None: not asserted)
PATHS = [("lean", {"VELO_SMALL_SOLVE": "0", "VELO_LM_LEAN": "1", "VELO_LM_SLIM": "0"}, 2, "eval_step_batch_lean_v_kernel"),
         ("lean_slim", {"VELO_SMALL_SOLVE": "0", "VELO_LM_LEAN": "1", "VELO_LM_SLIM": "1"}, 2, "eval_step_batch_lean_v_slim_kernel"),
         ("plain", {"VELO_SMALL_SOLVE": "0", "VELO_LM_LEAN": "0"}, 2, "eval_step_batch_v_kernel"),
         ("lean_two_launch", {"VELO_SMALL_SOLVE": "0", "VELO_LM_LEAN": "1", "VELO_LM_FUSED": "0"}, 2, None),
         ("single", {"VELO_SMALL_SOLVE": "0"}, 1, "lm_iter_kernel"),
         ("one_launch_solve", {"VELO_SMALL_SOLVE": "1"}, 1, "lm_solve_small_icp_kernel"),
         ("host", {"VELO_SMALL_SOLVE": "0", "VELO_CHAIN": "0"}, 1, None)]
SWITCHES = ("VELO_SMALL_SOLVE", "VELO_LM_LEAN", "VELO_LM_SLIM", "VELO_LM_FUSED", "VELO_CHAIN")


def register_on_every_path(diag_lib, monkeypatch, d):
    out = {}
    for name, env, n, kernel in PATHS:
        for k in SWITCHES:
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        ctxs = [api.Context(0, lib=diag_lib, icp_skip=1) for _ in range(n)]       # (the switches are read when a context is created)
        for c in ctxs:
            load(c, d)
        ctxs[0].set_timing(2)                                                     # launches counted by kernel name (a group's on its first context)
        res = []
        for rep in range(2):                                                      # the second call chains from real history
            if n == 1:
                x, T, s = ctxs[0].frame_to_frame(d["x0"])
                xs, Ts, Ss = [x], [T], [s]
            else:
                xs, Ts, Ss = api.register_batch(ctxs, None, None, [d["x0"]] * n)
            for i in range(n):
                res.append((np.array(xs[i], copy=True), np.array(Ts[i], copy=True).reshape(4, 4), summary_tuple(Ss[i])))
        out[name] = res
        launched = set(ctxs[0].kernel_times())
        assert kernel is None or kernel in launched, (name, kernel, sorted(launched))
        for c in ctxs:
            c.close()
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    x0, T0, s0 = out["host"][0]
    for name, res in out.items():
        for x, T, s in res:
            assert np.array_equal(x, x0) and np.array_equal(T, T0) and s == s0, (name, x, x0, s, s0)
    return x0, s0


@pytest.mark.parametrize("n", SIZES)
def test_row_counts_on_every_path(hip_lib, diag_lib, oracle, monkeypatch, pair, n):
    d = cut(pair, n)
    c = api.Context(0, icp_skip=1)
    orc = oracle.Oracle(threads=4, icp_skip=1)
    H.load_both(c, orc, d)
    check_evaluation(c, orc, d)
    c.close()
    x, s = register_on_every_path(diag_lib, monkeypatch, d)
    assert len(s) == 6 and np.all(np.isfinite(x))


def test_query_shard_that_does_not_start_at_zero(hip_lib, oracle, pair):
    d = cut(pair, SIZES[-1])
    c = api.Context(0, icp_skip=1)
    load(c, d)
    try:
        for rank, world in ((1, 3), (2, 3), (6, 7)):
            orc = oracle.Oracle(threads=4, icp_skip=1)
            orc.set_query_shard(rank, world)
            orc.set_target(d["tgt_xyz"], d["tgt_off"]); orc.set_source(d["src_xyz"], d["src_off"])
            c.set_query_shard(rank, world)
            assert check_evaluation(c, orc, d) > 0
    finally:
        c.set_query_shard(0, 1)
        c.close()


def validity_patterns(n):
    i = np.arange(n)
    nthreads = -(-n // ROWS_PER_BLOCK) * 256                                       # the sweep's stride: row k of thread t is query t + k nthreads
    return {"every_other_row": i[(i // nthreads) % 2 == 1],                        # rows 1 and 3 of every thread
            "every_other_query": i[i % 2 == 1],                                    # every other lane of every wave
            "whole_threads": i[np.isin(i % nthreads, (0, 5, 63, 64, 300, nthreads - 1))],
            "whole_workgroup": i[(i % nthreads) // 256 == 1],
            "first_rows": i[i < nthreads]}                                         # the prefetched row of every thread


@pytest.mark.parametrize("pattern", ["every_other_row", "every_other_query", "whole_threads", "whole_workgroup", "first_rows"])
def test_invalid_rows_between_valid_ones(hip_lib, diag_lib, oracle, monkeypatch, pair, pattern):
    n = SIZES[-1]
    bad = validity_patterns(n)[pattern]
    assert 0 < len(bad) < n
    d = cut(pair, n, invalid=bad)
    c = api.Context(0, icp_skip=1)
    orc = oracle.Oracle(threads=4, icp_skip=1)
    H.load_both(c, orc, d)
    nv = check_evaluation(c, orc, d)
    corr = c.correspondences()
    assert not corr["valid"][bad].any() and 0 < nv <= n - len(bad)                 # the moved sources found nothing inside the gate
    c.close()
    register_on_every_path(diag_lib, monkeypatch, d)


def test_pose_record_reaches_the_next_association_round(hip_lib, oracle, monkeypatch):
    """A chained call on the golden mini pair: every round after the first takes its pose from the record the previous solve's last LM
    launch left on the device.  Poses and solve logs equal the host-driven path's bit for bit, on the single-pair chain and on a lock-step
    group's, no call falls back (chain misses 0), and the pose is the oracle's."""
    m = dict(np.load(os.path.join(os.path.dirname(__file__), "golden", "mini_pair.npz")))
    d = dict(tgt_xyz=m["tgt_xyz"], tgt_off=m["tgt_off"], src_xyz=m["src_xyz"], src_off=m["src_off"], x0=synth.INITIAL_GUESS.copy())
    res, stats = {}, {}
    for name, chain, n in (("host", "0", 1), ("chain", "1", 1), ("host_group", "0", 2), ("chain_group", "1", 2)):
        monkeypatch.setenv("VELO_CHAIN", chain)
        ctxs = [api.Context(0, icp_skip=1) for _ in range(n)]
        for c in ctxs:
            load(c, d)
        out = []
        for rep in range(3):
            if n == 1:
                x, T, s = ctxs[0].frame_to_frame(d["x0"])
                out.append((x.copy(), T.copy(), summary_tuple(s)))
            else:
                xs, Ts, Ss = api.frame_to_frame_batch(ctxs, [d["x0"]] * n)
                out += [(np.array(xs[i], copy=True), np.array(Ts[i], copy=True).reshape(4, 4), summary_tuple(Ss[i])) for i in range(n)]
        res[name], stats[name] = out, [c.chain_stats() for c in ctxs]
        for c in ctxs:
            c.close()
    monkeypatch.delenv("VELO_CHAIN", raising=False)
    assert stats["host"] == [(0, 0)] and stats["host_group"] == [(0, 0)] * 2
    assert stats["chain"] == [(3, 0)] and stats["chain_group"] == [(3, 0)] * 2      # three chained calls each, none repeated
    x0, T0, s0 = res["host"][0]
    assert len(s0) == 6                                                            # six solves: five of them start from a pose record
    for name in res:
        for x, T, s in res[name]:
            assert np.array_equal(x, x0) and np.array_equal(T.reshape(4, 4), T0.reshape(4, 4)) and s == s0, name
    orc = oracle.Oracle(threads=4, icp_skip=1)
    orc.set_target(d["tgt_xyz"], d["tgt_off"]); orc.set_source(d["src_xyz"], d["src_off"])
    xo, _, so = orc.frame_to_frame(d["x0"])
    assert H.pose_close(x0, xo)
    assert [t[2] for t in s0] == [so.solves[k].evaluations for k in range(6)]


@pytest.mark.parametrize("shrunk", [False, True])
def test_default_choice_of_the_lean_launch_follows_the_grid(hip_lib, diag_lib, monkeypatch, pair, shrunk):
    """No VELO_LM_LEAN / VELO_LM_SLIM: four contexts are two lock-step groups sharing the chip, so their LM launches are lean ones.  On a
    regular grid they are the chunked launch; on a density-shrunk grid (VELO_DENSE_REF=50 makes this 4,800-point target "dense": the gate
    spans ~10 cells, shrunk_grid) they are the 126-VGPR one -- what a scan-to-map group gets -- and give, on that same grid, the bits of
    the chunked launch (VELO_LM_SLIM=0)."""
    d = cut(pair, SIZES[-1])
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("VELO_SMALL_SOLVE", "0")
    if shrunk:
        monkeypatch.setenv("VELO_DENSE_REF", "50")
    out = {}
    for slim in ([None, "0"] if shrunk else [None]):
        if slim is not None:
            monkeypatch.setenv("VELO_LM_SLIM", slim)
        ctxs = [api.Context(0, lib=diag_lib, icp_skip=1) for _ in range(4)]
        for c in ctxs:
            load(c, d)
            c.set_timing(2)
        xs, Ts, Ss = api.register_batch(ctxs, None, None, [d["x0"]] * 4)
        launched = set().union(*[set(c.kernel_times()) for c in ctxs])
        out[slim] = (launched, [(np.array(xs[i], copy=True), summary_tuple(Ss[i])) for i in range(4)])
        for c in ctxs:
            c.close()
    monkeypatch.delenv("VELO_DENSE_REF", raising=False)
    monkeypatch.delenv("VELO_LM_SLIM", raising=False)
    slim_name, chunked_name = "eval_step_batch_lean_v_slim_kernel", "eval_step_batch_lean_v_kernel"
    launched = out[None][0]
    if not shrunk:
        assert chunked_name in launched and slim_name not in launched, sorted(launched)
        return
    assert slim_name in launched and chunked_name not in launched, sorted(launched)
    assert chunked_name in out["0"][0] and slim_name not in out["0"][0], sorted(out["0"][0])
    for (x, s), (x0, s0) in zip(out[None][1], out["0"][1]):
        assert np.array_equal(x, x0) and s == s0

# ---- more than four rows per thread: a process of its own (the plan's rows per thread are read once per process) -----------------------
MORE_ROWS = "8"


class _Env:
    """monkeypatch's two calls, on the child's own environment"""
    def setenv(self, k, v):
        os.environ[k] = v

    def delenv(self, k, raising=False):
        os.environ.pop(k, None)


def sums_at_the_guess(lib, d):
    c = api.Context(0, lib=lib, icp_skip=1)
    load(c, d)
    c.associate(d["x0"], 1)
    cost, Hm, g = c.evaluate(d["x0"])
    c.close()
    return np.concatenate([[cost], Hm.ravel(), g]).tobytes().hex()


def more_rows_per_thread():
    import oracle_lib
    api.load_library()
    diag = api.load_diagnostics_library()
    n = SIZES[-1]
    pair = synth.scan_pair(n_beams=16, n_azimuth=300)
    whole = cut(pair, n)
    print("sums", sums_at_the_guess(diag, whole))
    for d in (whole, cut(pair, n, invalid=np.arange(1, n, 2))):
        c = api.Context(0, lib=diag, icp_skip=1)
        load(c, d)
        for rank, world in ((0, 1), (1, 2)):                   # 2 x 256 threads with 6-7 rows, then the second half of the list: 256 threads with 6
            orc = oracle_lib.Oracle(threads=4, icp_skip=1)
            orc.set_query_shard(rank, world)
            orc.set_target(d["tgt_xyz"], d["tgt_off"]); orc.set_source(d["src_xyz"], d["src_off"])
            c.set_query_shard(rank, world)
            assert check_evaluation(c, orc, d) > 0
        c.set_query_shard(0, 1)
        c.close()
        register_on_every_path(diag, _Env(), d)
    print("more rows: ok")


def test_more_rows_per_thread_than_the_first_chunk_holds(hip_lib, diag_lib, pair):
    """VELO_EVAL_PER_THREAD=8: 3,073 queries in 2 workgroups, six or seven rows per thread.  The lean launches sweep row 0 (prefetched),
    the chunk requested ahead (rows 1-3) and a chunk requested inside the loop (rows 4-6); the kernels with four prefetched rows take
    their chunked tail (rows 4-6), also from a shard whose first query is not 0.  Same assertions as above, in the child."""
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env["VELO_EVAL_PER_THREAD"] = MORE_ROWS
    out = subprocess.run([sys.executable, os.path.abspath(__file__)], env=env, capture_output=True, text=True, timeout=240)
    assert out.returncode == 0 and "more rows: ok" in out.stdout, out.stdout[-1500:] + out.stderr[-2500:]
    # the switch took: another partition of the rows sums in another order (the same plan would give the same bits)
    theirs = [l.split()[1] for l in out.stdout.splitlines() if l.startswith("sums ")]
    assert len(theirs) == 1 and theirs[0] != sums_at_the_guess(diag_lib, cut(pair, SIZES[-1]))


if __name__ == "__main__":
    assert os.environ.get("VELO_EVAL_PER_THREAD") == MORE_ROWS
    more_rows_per_thread()
