"""-m gpu: the LM sweep kernels against the sums of the commit BEFORE the workgroup reduction made its two lane exchanges with lane swaps
(block_reduce_store, which every LM kernel calls -- so agreement between the paths proves nothing any more, and the yardstick is a
recording).  The cases are also those a sweep that takes the eval point's matrices as scalar operands has to pass (EXPERIMENTS.md).

tests/golden/lm_parent_sums.npz holds, for every case below, what that commit's build gave on the GPU: the pose, the 4 x 4 transform, every
solve's initial and final cost (float64) and its termination, iteration, evaluation and valid-row counts (int64).  Every LM step is a
function of a launch's 21 + 6 sums and its cost, so a sum that changed in its last bit shows in them.  The cases (all on
synth.scan_pair(n_beams=16, n_azimuth=300), cut like tests/test_gpu_lm_row_loads.py cuts it):

  row counts   1, 255, 256, 257, 1023, 1025 and 3,073 queries: threads with no row, one, some and four, a last workgroup partly empty;
  paths        lean, slim (126 VGPRs), plain, the lean one-launch iteration, the single-pair iteration and the host-driven two-launch
               path; which kernel ran is asserted from the launch log.  Every solve's first launch builds its eval point in LDS, the
               later ones load it, and a chained call launches past the end of its solves (the margin on the predicted count), twice per
               path: the second call chains from real history;
  a group      two contexts with different pairs, sizes and guesses in one lock-step group, each against its single call and the
               recording (a scalar taken from the other context, or from an earlier launch, shows here), in either slot of the lean, the
               slim and the lean one-launch-iteration launches, and as two groups of two on the product library, which chooses its
               kernels itself (at these sizes one workgroup per solve: the same reduction);
  visual       the same group with 16 stereo matches in each context: the lean launch whose visual workgroups skip the row section;
  validity     every other row of every thread invalid, and every row of one whole workgroup.

velo_evaluate's cost and sums are checked against the oracle within the 1e-12 the parity tests use.  Nothing here looks at machine code.

Recording (on a GPU, with the build of the commit to record):  python tests/test_gpu_lm_scalar_matrices.py --record [file]"""
import os
import sys

import numpy as np
import pytest

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "tests")]
    import torch  # noqa: F401

import helpers as H
from velo_amd import api, synth
from test_gpu_lm_row_loads import SIZES, SWITCHES, check_evaluation, cut, load, summary_tuple, validity_patterns

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lm_parent_sums.npz")
ALL_SWITCHES = SWITCHES + ("VELO_LM_ITER",)
BASE = {"VELO_SMALL_SOLVE": "0"}
# (name, environment of the diagnostics build, contexts in the call, the LM kernel the launch log must name -- None: not asserted)
PATHS = [("lean", dict(BASE, VELO_LM_LEAN="1", VELO_LM_SLIM="0"), 2, "eval_step_batch_lean_v_kernel"),
         ("slim", dict(BASE, VELO_LM_LEAN="1", VELO_LM_SLIM="1"), 2, "eval_step_batch_lean_v_slim_kernel"),
         ("plain", dict(BASE, VELO_LM_LEAN="0"), 2, "eval_step_batch_v_kernel"),
         ("lean_iter", dict(BASE, VELO_LM_LEAN="1", VELO_LM_ITER="1"), 2, "lm_iter_batch_lean_kernel"),
         ("single", dict(BASE), 1, "lm_iter_kernel"),
         ("host", dict(BASE, VELO_CHAIN="0"), 1, None)]                 # (its launches are not logged by name)
LEAN = PATHS[0][1]


class _Env:
    """monkeypatch's two calls on this process's environment (the recording run has no monkeypatch)"""
    def setenv(self, k, v):
        os.environ[k] = v

    def delenv(self, k, raising=False):
        os.environ.pop(k, None)


def as_arrays(x, T, s):
    t = summary_tuple(s)
    return {"x": np.array(x, dtype=np.float64).reshape(6), "T": np.array(T, dtype=np.float64).reshape(16),
            "cost": np.array([[u[4], u[5]] for u in t], dtype=np.float64).reshape(-1, 2),
            "count": np.array([[u[0], u[1], u[2], u[3]] for u in t], dtype=np.int64).reshape(-1, 4)}


def run(lib, menv, env, datas, vis=None, reps=2, batch=True):
    """len(datas) contexts created under env on lib, context i loaded with datas[i], registered reps times in one call (batch) or by
    frame_to_frame; -> ([per rep: per context: arrays], the kernels the contexts launched)"""
    for k in ALL_SWITCHES:
        menv.delenv(k, raising=False)
    for k, v in env.items():
        menv.setenv(k, v)
    ctxs = [api.Context(0, lib=lib, icp_skip=1) for _ in datas]
    for k in ALL_SWITCHES:
        menv.delenv(k, raising=False)
    out = []
    try:
        for i, (c, d) in enumerate(zip(ctxs, datas)):
            load(c, d)
            if vis is not None:
                c.set_visual(vis[i])
            c.set_timing(2)
        for rep in range(reps):
            if batch:
                xs, Ts, Ss = api.register_batch(ctxs, None, None, [d["x0"] for d in datas])
                out.append([as_arrays(xs[i], Ts[i], Ss[i]) for i in range(len(ctxs))])
            else:
                res = []
                for c, d in zip(ctxs, datas):
                    x, T, s = c.frame_to_frame(d["x0"])
                    res.append(as_arrays(x, T, s))
                out.append(res)
        launched = set().union(*[set(c.kernel_times()) for c in ctxs])
    finally:
        for c in ctxs:
            c.close()
    return out, launched


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("x", "T", "cost", "count"))


def base_pair():
    d = synth.scan_pair(n_beams=16, n_azimuth=300)
    assert len(d["src_xyz"]) >= SIZES[-1]
    return d


def group_datas(pair):
    """two contexts of one lock-step group: different scenes, row counts (4 workgroups against 2, the second partly empty) and guesses"""
    other = synth.scan_pair(n_beams=16, n_azimuth=300, scene_seed=7, sigma=0.03)
    b = cut(other, 1025)
    b["x0"] = np.array([0.004, -0.006, 0.002, 0.05, -0.03, 0.8])
    return [cut(pair, SIZES[-1]), b]


def group_visual(datas):
    return [api.matches_from_dict(synth.stereo_matches(8, seed=21 + i, mix="all", x_true=d["x_true"])) for i, d in enumerate(datas)]


def validity_cases(pair):
    n = SIZES[-1]
    pat = validity_patterns(n)
    return {"invalid_every_other_row": cut(pair, n, invalid=pat["every_other_row"]),
            "invalid_whole_workgroup": cut(pair, n, invalid=pat["whole_workgroup"])}


def record(path):
    """what the build in the tree gives for every case -> path.  The row-count and validity cases are run on every path and must agree bit
    for bit (at the commit this is meant to run on they do: tests/test_gpu_lm_row_loads.py); the group's contexts one by one, host-driven."""
    api.load_library()
    diag = api.load_diagnostics_library()
    pair, env, out = base_pair(), _Env(), {}
    host = PATHS[-1][1]

    def put(name, arrs):
        for k, v in arrs.items():
            out[f"{name}/{k}"] = v

    singles = {f"n{n}": cut(pair, n) for n in SIZES}
    singles.update(validity_cases(pair))
    for name, d in singles.items():
        for pname, penv, nctx, kernel in PATHS:                  # the recording is only worth something where the paths agree
            res, launched = run(diag, env, penv, [d] * nctx)
            assert kernel is None or kernel in launched, (name, pname, sorted(launched))
            if pname == "lean":
                first = res[0][0]
            assert all(same(r, first) for rep in res for r in rep), (name, pname)
        put(name, first)
    datas = group_datas(pair)
    for i, d in enumerate(datas):
        res, _ = run(diag, env, host, [d], batch=False)
        put(f"group{i}", res[0][0])
    vis = group_visual(datas)
    for i, d in enumerate(datas):
        res, _ = run(diag, env, host, [d], vis=[vis[i]], batch=False)
        put(f"group_visual{i}", res[0][0])
    np.savez_compressed(path, **out)
    print("recorded", len(out), "arrays,", os.path.getsize(path), "bytes")


@pytest.fixture(scope="module")
def pair():
    return base_pair()


@pytest.fixture(scope="module")
def golden():
    g = np.load(GOLDEN)
    return lambda name: {k: g[f"{name}/{k}"] for k in ("x", "T", "cost", "count")}


def assert_paths_equal_recording(diag_lib, monkeypatch, d, want):
    assert want["count"].shape == (6, 4) and np.all(np.isfinite(want["x"]))
    for pname, penv, nctx, kernel in PATHS:
        res, launched = run(diag_lib, monkeypatch, penv, [d] * nctx)
        assert kernel is None or kernel in launched, (pname, kernel, sorted(launched))
        for rep in res:
            for got in rep:
                assert same(got, want), (pname, got, want)


@pytest.mark.parametrize("n", SIZES)
def test_row_counts_on_every_path_equal_the_recording(hip_lib, diag_lib, oracle, monkeypatch, pair, golden, n):
    d = cut(pair, n)
    c = api.Context(0, icp_skip=1)
    orc = oracle.Oracle(threads=4, icp_skip=1)
    H.load_both(c, orc, d)
    check_evaluation(c, orc, d)                                   # cost and the 21 + 6 sums of velo_evaluate: 1e-12 of the oracle's
    c.close()
    assert_paths_equal_recording(diag_lib, monkeypatch, d, golden(f"n{n}"))


@pytest.mark.parametrize("pattern", ["every_other_row", "whole_workgroup"])
def test_invalid_rows_equal_the_recording(hip_lib, diag_lib, oracle, monkeypatch, pair, golden, pattern):
    d = validity_cases(pair)[f"invalid_{pattern}"]
    c = api.Context(0, icp_skip=1)
    orc = oracle.Oracle(threads=4, icp_skip=1)
    H.load_both(c, orc, d)
    assert check_evaluation(c, orc, d) > 0
    c.close()
    assert_paths_equal_recording(diag_lib, monkeypatch, d, golden(f"invalid_{pattern}"))


def test_group_of_different_pairs_and_guesses(hip_lib, diag_lib, monkeypatch, pair, golden):
    datas = group_datas(pair)
    want = [golden("group0"), golden("group1")]
    assert not same(want[0], want[1])
    singles, launched = run(diag_lib, monkeypatch, PATHS[4][1], datas, batch=False)
    assert "lm_iter_kernel" in launched
    for pname in ("lean", "slim", "lean_iter"):
        _, penv, _, kernel = [p for p in PATHS if p[0] == pname][0]
        for order in (datas, datas[::-1]):                        # either context in either slot of the launch
            res, launched = run(diag_lib, monkeypatch, penv, order)
            assert kernel in launched, (pname, sorted(launched))
            w = want if order is datas else want[::-1]
            s = singles[0] if order is datas else singles[0][::-1]
            for rep in res:
                for i in range(2):
                    assert same(rep[i], w[i]) and same(rep[i], s[i]), (pname, i, rep[i], w[i])
    # the product library's own choice for two groups of two (at these sizes a one-workgroup solve per context: the same reduction)
    res, launched = run(None, monkeypatch, {}, datas + datas[::-1])
    assert any(k.startswith("lm_") or k.startswith("eval_step") for k in launched), sorted(launched)
    for rep in res:
        for got, w in zip(rep, want + want[::-1]):
            assert same(got, w)


def test_group_with_visual_blocks(hip_lib, diag_lib, monkeypatch, pair, golden):
    datas = group_datas(pair)
    vis = group_visual(datas)
    assert all(len(v) == 16 for v in vis)
    want = [golden("group_visual0"), golden("group_visual1")]
    assert not same(want[0], golden("group0"))                    # the blocks took part
    singles, _ = run(diag_lib, monkeypatch, PATHS[4][1], datas, vis=vis, batch=False)
    res, launched = run(diag_lib, monkeypatch, LEAN, datas, vis=vis)
    assert "eval_step_batch_lean_vis_kernel" in launched, sorted(launched)
    for rep in res:
        for i in range(2):
            assert same(rep[i], want[i]) and same(rep[i], singles[0][i]), (i, rep[i], want[i])
    res, launched = run(None, monkeypatch, {}, (datas + datas[::-1]), vis=vis + vis[::-1])
    assert any(k.startswith("lm_") or k.startswith("eval_step") for k in launched), sorted(launched)
    for rep in res:
        for got, w in zip(rep, want + want[::-1]):
            assert same(got, w)


if __name__ == "__main__":
    assert sys.argv[1] == "--record" and len(sys.argv) <= 3
    record(sys.argv[2] if len(sys.argv) == 3 else GOLDEN)
