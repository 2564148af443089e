"""The bundle adjustment's part of the drop-in boundary (no GPU): the structs of include/velo_hip.h against the ctypes mirror of
api.py, the status constants, and the entry points' behaviour that needs no device."""
import ctypes as C
import os
import subprocess

import pytest

import velo_amd  # noqa: F401
from velo_amd import api, build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROBE = r'''
#include <stdio.h>
#include <stddef.h>
#include "velo_hip.h"
int main(void) {
  printf("%zu %zu %zu\n", sizeof(velo_ba_params), sizeof(velo_ba_iteration), sizeof(velo_ba_summary));
  printf("%zu %zu\n", offsetof(velo_ba_params, weight_3d), offsetof(velo_ba_params, reserved));
  printf("%zu %zu %zu %zu %zu %zu %zu\n", offsetof(velo_ba_iteration, status), offsetof(velo_ba_iteration, iteration), offsetof(velo_ba_iteration, cost),
         offsetof(velo_ba_iteration, candidate_cost), offsetof(velo_ba_iteration, radius), offsetof(velo_ba_iteration, model_change),
         offsetof(velo_ba_iteration, step_norm));
  printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", offsetof(velo_ba_summary, termination), offsetof(velo_ba_summary, iterations),
         offsetof(velo_ba_summary, evaluations), offsetof(velo_ba_summary, n_landmarks), offsetof(velo_ba_summary, n_blocks),
         offsetof(velo_ba_summary, n_residuals), offsetof(velo_ba_summary, n_trace), offsetof(velo_ba_summary, initial_cost),
         offsetof(velo_ba_summary, final_cost), offsetof(velo_ba_summary, trace));
  printf("%d %d %d %d %d %d %d %d\n", VELO_BA_MAX_FREE, VELO_BA_MAX_TRACE, VELO_BA_ACCEPTED, VELO_BA_REJECTED, VELO_BA_INVALID, VELO_BA_PARAMETER,
         VELO_BA_FUNCTION, VELO_BA_GRADIENT);
  return 0; }
'''


def test_struct_layouts_match_the_ctypes_mirror(tmp_path):
    cfile, exe = str(tmp_path / "probe.c"), str(tmp_path / "probe")
    open(cfile, "w").write(PROBE)
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), cfile, "-o", exe], check=True)      # the header is plain C
    rows = [[int(v) for v in line.split()] for line in subprocess.run([exe], check=True, capture_output=True, text=True).stdout.splitlines()]
    P, I, S = api.VeloBaParams, api.VeloBaIteration, api.VeloBaSummary
    assert rows[0] == [C.sizeof(P), C.sizeof(I), C.sizeof(S)] == [16, 48, 48 + 50 * 48]
    assert rows[1] == [P.weight_3d.offset, P.reserved.offset]
    assert rows[2] == [getattr(I, n).offset for n in ("status", "iteration", "cost", "candidate_cost", "radius", "model_change", "step_norm")]
    assert rows[3] == [getattr(S, n).offset for n in ("termination", "iterations", "evaluations", "n_landmarks", "n_blocks", "n_residuals", "n_trace",
                                                      "initial_cost", "final_cost", "trace")]
    assert rows[4] == [api.BA_MAX_FREE, api.BA_MAX_TRACE, api.BA_ACCEPTED, api.BA_REJECTED, api.BA_INVALID, api.BA_PARAMETER, api.BA_FUNCTION, api.BA_GRADIENT]


@pytest.fixture(scope="module")
def lib():
    build.build_hip()
    return api.load_library()


def test_default_params_and_null_arguments(lib):
    p = api.VeloBaParams()
    p.weight_3d = 7.0
    assert lib.velo_default_ba_params(C.byref(p)) == 0
    assert p.weight_3d == 1.0 and list(p.reserved) == [0, 0]
    assert lib.velo_default_ba_params(None) == -1
    # refused before a context is looked at
    assert lib.velo_landmarks_adjust(None, None, 2, 1, None, None, None) == -1
    assert lib.velo_landmarks_adjust_system(None, None, 2, 1, None, None, None, None) == -1
