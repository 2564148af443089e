"""tests/pose_graph_cov_ref.py, the restatement of velo_graph_covariance, checked on its own (no GPU): on every graph of the GPU
test its three routes to Sigma = (J^T J)^-1 -- the inverse, the QR of J, the Takahashi recursion over the envelope -- against each
other, at the loaded state; the largest pairwise difference, normalised by sigma_i sigma_j, is what
tests/test_gpu_pose_graph_covariance.py derives its tolerances from.  The Takahashi route must never read a block outside the
envelope.  Also what of the new entry needs no device: the refusals of a null context and the two forms of Context.graph_covariance's
first argument."""
import ctypes as C
import functools

import numpy as np
import pytest

import pose_graph_cov_ref as R
import velo_amd  # noqa: F401
from velo_amd import api, build

# Measured here: the largest spread between two of the three routes, over every block inside the envelope (all three) and over the whole
# matrix (inverse against QR).  free1 has one 6 x 6 and the routes agree to a few units of the format.
SPREAD = {"free1": 4.4e-16, "free2": 5.2e-16, "chain5": 1.2e-15, "large_rotation": 1.0e-15, "ring70": 9.6e-13, "chain250": 2.7e-10,
          "chain250_split": 3.6e-11, "lap454": 5.9e-11, "hub140": 2.8e-13, "ring70_outliers": 9.6e-14, "chain5_mixed": 4.1e-15}


@functools.lru_cache(maxsize=None)
def routes(name):
    g, prob = R.fixture(name)
    J = R.dense_jacobian(prob)
    ea, eb = R.free_edges(g, prob)
    return g, prob, R.by_inverse(J), R.by_qr(J), R.Takahashi(J, prob.n_free, ea, eb)


def measure(name):
    _, prob, S1, S2, T = routes(name)
    sigma = np.sqrt(np.diag(S1))
    full = float(np.max(np.abs(S1 - S2) / np.outer(sigma, sigma)))
    env, blocks = 0.0, 0
    for hi in range(T.n):
        for lo in range(int(T.first[hi]), hi + 1):
            a, b = int(T.perm[hi]), int(T.perm[lo])
            Z = T.block(a, b)
            sa, sb = sigma[6 * a:6 * a + 6], sigma[6 * b:6 * b + 6]
            env = max(env, R.cov_spread(Z, R.block_of(S1, a, b), sa, sb), R.cov_spread(Z, R.block_of(S2, a, b), sa, sb))
            blocks += 1
    return full, env, blocks, T


@pytest.mark.parametrize("name", R.FIXTURES)
def test_the_three_routes_agree(name):
    full, env, blocks, T = measure(name)
    _, prob, S1, _, _ = routes(name)
    print(f"{name}: inverse against QR {full:.2e}, Takahashi against both {env:.2e} over {blocks} blocks (record {SPREAD[name]:.1e}); "
          f"{prob.n_free} free nodes, widest row {T.stats[0]}, {T.stats[3]} components")
    assert T.outside_reads == 0                                        # the envelope is closed under the recursion
    assert blocks == T.stats[1]
    assert max(full, env) <= 3 * SPREAD[name]                          # the record is what was measured, to a factor of 3 (LAPACK builds differ)


def test_what_the_fixtures_are_for():
    T = {name: routes(name)[4] for name in R.FIXTURES}
    assert T["free1"].n == 1 and T["free2"].n == 2
    assert np.any(np.diff(T["chain250"].first) < 0)                    # `first` is not monotone
    assert T["chain250_split"].stats[3] == 2
    assert T["lap454"].stats[0] >= 26 - 1                              # a column of 26 rows: 676 block products, several per thread group
    assert T["hub140"].stats[0] + 1 >= 128 and T["hub140"].stats[3] == 1
    for name in ("ring70", "chain250", "chain250_split", "lap454", "hub140", "ring70_outliers"):
        pairs = R.outside_pairs(T[name].perm, T[name].first)
        assert len(pairs) == 3 and all(not T[name].inside(a, b) for a, b in pairs), name
    # across the two components of chain250_split the covariance is zero, and such a pair lies outside the envelope
    g, prob, S1, _, _ = routes("chain250_split")
    assert np.max(np.abs(R.block_of(S1, prob.slot[100], prob.slot[200]))) <= 1e-30
    assert not T["chain250_split"].inside(prob.slot[100], prob.slot[200])


def test_the_order_of_the_restatement_is_the_librarys():
    for name in ("chain250", "lap454", "hub140"):
        g, prob, _, _, T = routes(name)
        ea, eb = R.free_edges(g, prob)
        perm, first, stats = api.graph_order(prob.n_free, ea, eb)
        assert np.array_equal(perm, T.perm) and np.array_equal(first, T.first)
        assert (stats["widest_row"], stats["envelope_blocks"], stats["work"], stats["components"]) == tuple(T.stats)


@pytest.fixture(scope="module")
def lib():
    return C.CDLL(build.build_hip())


def test_refusals_that_need_no_device(lib):
    one = (C.c_int32 * 1)(0)
    out = (C.c_double * 36)(*([7.0] * 36))
    lib.velo_last_error.restype = C.c_char_p
    lib.velo_graph_covariance.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    assert lib.velo_graph_covariance(None, one, 1, None, 1, one, one, out) == -1 and b"null ctx" in lib.velo_last_error()
    assert lib.velo_graph_covariance(None, None, 0, None, 0, None, None, None) == -1 and b"null ctx" in lib.velo_last_error()
    assert all(v == 7.0 for v in out)


class _Recorder:
    """stands in for a context: keeps what Context.graph_covariance hands to the C-ABI and fills every block with its pair's frames"""

    def __init__(self):
        self._h, self.calls = None, []
        self._lib = self
        self._graph_params = api.Context._graph_params

    def _check(self, status):
        assert status == 0

    def velo_graph_covariance(self, h, fixed, n_fixed, params, n, a, b, out):
        fa = np.ctypeslib.as_array(C.cast(a, C.POINTER(C.c_int32)), (n,)).copy() if n else np.zeros(0, np.int32)
        fb = np.ctypeslib.as_array(C.cast(b, C.POINTER(C.c_int32)), (n,)).copy() if n else np.zeros(0, np.int32)
        fx = np.ctypeslib.as_array(C.cast(fixed, C.POINTER(C.c_int32)), (n_fixed,)).copy()
        self.calls.append((fa, fb, fx, params))
        blocks = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_double)), (max(n, 1) * 36,))
        for p in range(n):
            blocks[36 * p:36 * p + 36] = 100.0 * fa[p] + fb[p] + 0.01 * np.arange(36)
        return 0


def test_the_two_forms_of_the_python_argument():
    ctx = _Recorder()
    m = api.Context.graph_covariance(ctx, [3, 5, 9], fixed=(0, 2))
    fa, fb, fx, params = ctx.calls[-1]
    assert m.shape == (3, 6, 6) and np.array_equal(fa, [3, 5, 9]) and np.array_equal(fb, [3, 5, 9]) and np.array_equal(fx, [0, 2]) and params is None
    p = api.Context.graph_covariance(ctx, np.array([[3, 5], [5, 3]]), max_work=77)
    fa, fb, fx, params = ctx.calls[-1]
    assert p.shape == (2, 6, 6) and np.array_equal(fa, [3, 5]) and np.array_equal(fb, [5, 3]) and np.array_equal(fx, [0]) and params is not None
    assert p[0, 0, 0] == 305.0 and p[1, 0, 0] == 503.0 and p[0, 0, 1] == 305.01    # row-major blocks, in the order of the request
    assert api.Context.graph_covariance(ctx, []).shape == (0, 6, 6)
    for bad in ([[1, 2, 3]], np.zeros((2, 2, 2), dtype=np.int32), [1.5, 2.0]):
        with pytest.raises(ValueError):
            api.Context.graph_covariance(ctx, bad)
    # the joint covariance: one call of three blocks, the (b, a) block the transpose of the returned (a, b) block
    ctx.graph_covariance = lambda pairs, fixed=(0,), max_work=None: api.Context.graph_covariance(ctx, pairs, fixed, max_work)
    J = api.Context.graph_joint_covariance(ctx, 4, 8)
    fa, fb, _, _ = ctx.calls[-1]
    assert np.array_equal(fa, [4, 4, 8]) and np.array_equal(fb, [4, 8, 8])
    assert J.shape == (12, 12) and np.array_equal(J[6:, :6], J[:6, 6:].T) and J[0, 6] == 408.0 and J[6, 6] == 808.0 and J[0, 0] == 404.0
