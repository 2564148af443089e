"""The trust-region controller shared by triangulation, bundle adjustment and the pose graph (csrc/velo_trust_region.h) as a
stand-alone C++ program under the address and undefined-behaviour sanitizers (tests/cpp/test_trust_region.cpp): scripted solves
go in, the controller's state after every line comes out, and every field must equal this file's own restatement of SURVEY.md B1
(Ceres' documented defaults) -- the doubles bit for bit.  Every exit and branch of B1 has a script of its own.  No GPU, no library."""
import math
import os
import random
import struct
import subprocess

import pytest

from velo_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")

CONVERGENCE, NO_CONVERGENCE, FAILURE = 0, 1, 2                                   # include/velo_hip.h: VELO_*
ACCEPTED, REJECTED, INVALID, PARAMETER, FUNCTION, GRADIENT = 0, 1, 2, 3, 4, 5    # VELO_BA_*
ORDER = ("max_num_iterations", "max_invalid", "function_tolerance", "gradient_tolerance", "parameter_tolerance", "initial_radius",
         "max_radius", "min_radius", "min_relative_decrease", "min_diag", "max_diag")
CERES = dict(max_num_iterations=50, max_invalid=5, function_tolerance=1e-6, gradient_tolerance=1e-10, parameter_tolerance=1e-8,
             initial_radius=1e4, max_radius=1e16, min_radius=1e-32, min_relative_decrease=1e-3, min_diag=1e-6, max_diag=1e32)


def b1(P, start, lines):
    """SURVEY.md B1 on reduced numbers.  A line is "invalid" or (candidate cost, model change, |step|, |x|, max |g|); a row is
    (status, done, termination, iteration, evaluations, refresh, radius, decrease, cost) after the start and after every line, each
    taken after the head of the next iteration; the rows end with the solve."""
    cost, x_norm, g = start
    mu, nu, k, invalid, evaluations, refresh, status = P["initial_radius"], 2.0, 0, 0, 1, 1, 0
    end = CONVERGENCE if g <= P["gradient_tolerance"] else None
    rows = []
    for line in [None] + list(lines):
        if line == "invalid":
            status, invalid = INVALID, invalid + 1
            if invalid >= P["max_invalid"]: end = FAILURE
            else: mu, nu, refresh = mu / nu, 2.0 * nu, 0
        elif line is not None:
            cost_c, model_change, step, x_norm_c, g_c = line
            invalid, evaluations = 0, evaluations + 1
            q = (cost - cost_c) / model_change
            if step <= P["parameter_tolerance"] * (x_norm + P["parameter_tolerance"]): status, end = PARAMETER, CONVERGENCE
            elif abs(cost - cost_c) <= P["function_tolerance"] * cost: status, end = FUNCTION, CONVERGENCE
            elif q > P["min_relative_decrease"]:
                status, cost, x_norm = ACCEPTED, cost_c, x_norm_c
                if g_c <= P["gradient_tolerance"]: status, end = GRADIENT, CONVERGENCE
                else:
                    t = 2.0 * q - 1.0
                    mu, nu, refresh = min(P["max_radius"], mu / max(1.0 / 3.0, 1.0 - t * t * t)), 2.0, 1
            else: status, mu, nu, refresh = REJECTED, mu / nu, 2.0 * nu, 0
        if end is None:
            if k + 1 > P["max_num_iterations"]: end = NO_CONVERGENCE
            elif mu < P["min_radius"]: end = CONVERGENCE
            else: k += 1
        rows.append((status, int(end is not None), NO_CONVERGENCE if end is None else end, k, evaluations, refresh, mu, nu, cost))
        if end is not None: break
    return rows


def script_text(P, start, lines):
    h = lambda v: float(v).hex()
    out = ["solve %d %d " % (P["max_num_iterations"], P["max_invalid"]) + " ".join(h(P[k]) for k in ORDER[2:]), "start " + " ".join(h(v) for v in start)]
    out += ["invalid" if l == "invalid" else "step " + " ".join(h(v) for v in l) for l in lines]
    return "\n".join(out) + "\n"


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("trust_region") / "test_trust_region")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.dirname(build.LIB), os.path.join(CPP, "test_trust_region.cpp"), "-o", path], check=True)
    return path


def run(exe, scripts):
    """every script through ONE process; the restatement's rows of each, after they have been found equal to the program's"""
    out = subprocess.run([exe], input="".join(script_text(*s) for s in scripts), capture_output=True, text=True)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]
    got = [l.split() for l in out.stdout.splitlines()]
    want = [b1(*s) for s in scripts]
    assert len(got) == sum(len(w) for w in want)
    bits = lambda v: struct.pack("<d", v)
    at = 0
    for n, w in enumerate(want):
        for i, row in enumerate(w):
            g = got[at]
            at += 1
            assert [int(v) for v in g[:6]] == list(row[:6]), (n, i, g, row)
            assert [bits(float.fromhex(v)) for v in g[6:]] == [bits(v) for v in row[6:]], (n, i, g, row)
    return want


def params(**kw):
    return dict(CERES, **kw)


START = (1.0, 1.0, 1.0)
GOOD = (0.5, 0.5, 0.1, 1.0, 1.0)         # ratio 1: accepted, the radius triples
BAD = (2.0, 0.5, 0.1, 1.0, 1.0)          # the cost goes up: rejected


def test_gradient_exit_at_the_start(exe):
    for g, done in ((1e-10, 1), (math.nextafter(1e-10, 1.0), 0)):
        (rows,) = run(exe, [(CERES, (1.0, 1.0, g), [])])
        assert rows == [(0, done, CONVERGENCE if done else NO_CONVERGENCE, 1 - done, 1, 1, 1e4, 2.0, 1.0)]


def test_max_num_iterations_exit(exe):
    (rows,) = run(exe, [(params(max_num_iterations=3), START, [(0.5 ** (i + 1), 0.5 ** (i + 1), 0.1, 1.0, 1.0) for i in range(5)])])
    assert len(rows) == 4 and [r[3] for r in rows] == [1, 2, 3, 3] and rows[-1][:3] == (ACCEPTED, 1, NO_CONVERGENCE) and rows[-1][4] == 4
    (rows,) = run(exe, [(params(max_num_iterations=0), START, [GOOD])])
    assert rows == [(0, 1, NO_CONVERGENCE, 0, 1, 1, 1e4, 2.0, 1.0)]


def test_min_radius_exit_after_repeated_rejections(exe):
    (rows,) = run(exe, [(params(min_radius=1.0), START, [BAD] * 10)])
    assert [r[6] for r in rows] == [1e4, 5e3, 1250.0, 156.25, 156.25 / 16, 156.25 / 512]
    assert all(r[:3] == (REJECTED, 0, NO_CONVERGENCE) for r in rows[1:-1]) and rows[-1][:4] == (REJECTED, 1, CONVERGENCE, 5) and rows[-1][8] == 1.0


def test_failure_after_exactly_max_invalid_steps(exe):
    (rows,) = run(exe, [(CERES, START, ["invalid"] * 8)])
    assert len(rows) == 6 and all(r[:3] == (INVALID, 0, NO_CONVERGENCE) for r in rows[1:5]) and rows[5][:3] == (INVALID, 1, FAILURE)
    assert rows[5][4] == 1 and rows[5][6:8] == rows[4][6:8] == (1e4 / 1024, 32.0)     # nothing evaluated; the fifth does not shrink


def test_one_valid_step_resets_the_invalid_counter(exe):
    (rows,) = run(exe, [(CERES, START, ["invalid"] * 4 + [BAD] + ["invalid"] * 5)])
    assert len(rows) == 11 and [r[1] for r in rows] == [0] * 10 + [1] and rows[-1][:3] == (INVALID, 1, FAILURE) and rows[5][0] == REJECTED


def test_parameter_and_function_exits_on_their_boundaries(exe):
    edge = 1e-8 * (3.0 + 1e-8)
    at, past = run(exe, [(CERES, (1.0, 3.0, 1.0), [(0.5, 0.5, s, 3.0, 1.0)]) for s in (edge, math.nextafter(edge, 1.0))])
    assert at[1][:3] == (PARAMETER, 1, CONVERGENCE) and at[1][8] == 1.0 and past[1][:2] == (ACCEPTED, 0)
    P = params(function_tolerance=2.0 ** -20)                  # 1 - 2^-20 and its neighbour below are exact, and so are the cost changes
    at, past, up = run(exe, [(P, START, [(c, 1.0, 0.1, 1.0, 1.0)]) for c in (1.0 - 2.0 ** -20, math.nextafter(1.0 - 2.0 ** -20, 0.0), 1.0 + 2.0 ** -20)])
    assert at[1][:3] == (FUNCTION, 1, CONVERGENCE) and at[1][4] == 2 and past[1][:2] == (REJECTED, 0)
    assert up[1][:3] == (FUNCTION, 1, CONVERGENCE)             # fabs: a tiny increase ends the solve too


def test_accepted_then_gradient_exit(exe):
    (rows,) = run(exe, [(CERES, START, [(0.5, 0.5, 0.1, 1.0, 1e-10), GOOD])])
    assert rows[1] == (GRADIENT, 1, CONVERGENCE, 1, 2, 1, 1e4, 2.0, 0.5)         # the cost moves, the radius does not


def test_radius_growth_is_clamped_at_max_radius(exe):
    free, clamped = run(exe, [(params(max_radius=m), START, [GOOD]) for m in (1e16, 2e4)])
    assert free[1][6] == 1e4 / (1.0 / 3.0) and clamped[1][6] == 2e4 and clamped[1][0] == ACCEPTED


def test_rejected_sequence_then_accept(exe):
    (rows,) = run(exe, [(CERES, START, [BAD, BAD, BAD, GOOD])])
    assert [r[6:8] for r in rows[:4]] == [(1e4, 2.0), (5e3, 4.0), (1250.0, 8.0), (156.25, 16.0)] and [r[5] for r in rows] == [1, 0, 0, 0, 1]
    assert rows[4][0] == ACCEPTED and rows[4][7] == 2.0 and rows[4][6] == 156.25 / (1.0 / 3.0) and rows[4][8] == 0.5


def test_ratio_equal_to_min_relative_decrease_is_rejected(exe):
    P = params(min_relative_decrease=2.0 ** -10)
    at, above = run(exe, [(P, START, [(c, 1.0, 0.1, 1.0, 1.0)]) for c in (1.0 - 2.0 ** -10, math.nextafter(1.0 - 2.0 ** -10, 0.0))])
    assert at[1][0] == REJECTED and at[1][8] == 1.0 and above[1][0] == ACCEPTED


def test_random_scripts(exe):
    rng = random.Random(20260417)
    scripts, seen = [], set()
    for _ in range(200):
        P = params(max_num_iterations=rng.randint(1, 60), max_invalid=rng.randint(1, 5), max_radius=rng.choice([1e16, 1e16, 3e4, 1e5]),
                   min_radius=rng.choice([1e-32, 1e-32, 1e-3, 10.0]), function_tolerance=rng.choice([1e-6, 1e-6, 1e-3]))
        cost = rng.uniform(0.1, 100.0)
        start, lines = (cost, rng.uniform(0.0, 10.0), rng.choice([1.0, 1.0, 1e-3, 1e-11])), []
        for _ in range(rng.randint(0, 60)):
            if rng.random() < 0.2: lines.append("invalid")
            else:
                cost_c = cost * rng.choice([0.3, 0.9, 0.99, 0.9999, 1.0 - 1e-7, 1.0, 1.001, 1.5, 4.0]) * rng.uniform(0.999, 1.001)
                model_change = (abs(cost - cost_c) + 1e-12) * rng.choice([0.5, 1.0, 1.0, 2.0, 10.0, 2000.0])
                lines.append((cost_c, model_change, rng.choice([1.0, 0.1, 1e-3, 1e-9]), rng.uniform(0.0, 10.0), rng.choice([1.0, 1.0, 1.0, 1e-4, 1e-11])))
                if cost_c < cost and rng.random() < 0.9: cost = cost_c
        scripts.append((P, start, lines))
    for rows in run(exe, scripts):
        seen.update((r[0], r[2]) for r in rows[1:])
    assert {s for s, _ in seen} == {ACCEPTED, REJECTED, INVALID, PARAMETER, FUNCTION, GRADIENT} and {t for _, t in seen} == {CONVERGENCE, NO_CONVERGENCE, FAILURE}
