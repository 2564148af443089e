"""CPU: the CHOICES the oracle restates from velo.h, checked against what the reference's own text says -- recorded as data in
tests/golden/reference_facts.json by tests/golden/make_reference_facts.py, which reads a checkout of the reference (nothing of its text is
kept here; `--check` re-reads it).  Not a substitute for running the reference -- it cannot be built here -- but it
turns "as far as I can read it" into assertions a change of either side would trip:
which residual functor gets which loss, threshold and weight (velo.h:683-689,710-718,744-752,777-785,875-891), the strict '<' of the
ring scan and of the neighbour choice (velo.h:836,843,859), the query stride and the enable_icp multiplier (velo.h:806-807), and that
ceres::Solve runs on defaults except for the linear solver type (velo.h:897-902)."""
import json
import os

import numpy as np

import helpers as H
import oracle_lib as ol
import velo_amd  # noqa: F401
from velo_amd import synth

FACTS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_facts.json")
KIND = {"cost3D3D": 0, "cost3D2D": 1, "cost2D3D": 2, "cost2D2D": 3, "cost3DPD": 4}          # ResidualType order + the point-to-plane block


def _facts():
    return json.load(open(FACTS))


def _written(*names):
    """the recorded yes / no of every named line of the reference (make_reference_facts.as_written)"""
    f = _facts()["as_written"]
    return {n: f[n] for n in names if f[n] is not True}


def test_every_block_kind_carries_the_references_loss():
    sites = {name: tuple(v) for name, v in _facts()["loss_sites"].items()}
    assert set(sites) == set(KIND)
    assert sites["cost3D3D"] == (3, "ArctanLoss", "loss_thresh_3D3D", None)
    assert sites["cost3DPD"][1] == "CauchyLoss" and sites["cost2D2D"][1] == "ArctanLoss"
    # ... and the oracle's blocks say the same, kind by kind
    d = H.small_pair()
    vis = synth.stereo_matches(80, mix="all", outlier_frac=0.0, x_true=d["x_true"])
    o = ol.Oracle(icp_skip=1)
    o.set_target(d["tgt_xyz"], d["tgt_off"])
    o.set_source(d["src_xyz"], d["src_off"])
    o.set_visual(vis)
    o.build_visual(d["x0"], 1)
    o.associate(d["x0"], 1)
    blocks = o.blocks()
    P = o.params
    dims = {0: 3, 1: 2, 2: 2, 3: 1, 4: 1}
    for name, kind in KIND.items():
        dim, loss, thresh, weight = sites[name]
        b = blocks[blocks["kind"] == kind]
        assert len(b) > 0, name
        assert dim == dims[kind]
        assert np.all(b["loss_type"] == {"CauchyLoss": 1, "ArctanLoss": 2}[loss]), name
        assert np.all(b["loss_a"] == float(getattr(P, thresh))), (name, thresh)
        assert np.all(b["loss_w"] == (float(getattr(P, weight)) if weight else 1.0)), (name, weight)


def test_ring_scan_neighbour_choice_and_query_stride_as_written():
    # velo.h:836,843: strict '<' twice -- ties keep the lower ring; the second test is an else-if
    # velo.h:859: the +1 neighbour only when STRICTLY closer
    # velo.h:806-807: the ring loop bound is multiplied by enable_icp, the point loop strides by icp_skip from 0
    # velo.h:828-829: a ring counts when the search found something and the SQUARED distance is within the gate
    # velo.h:873: degenerate planes are skipped on the norm of the un-normalised normal
    assert _written("ring_scan_strict_less_then_else_if", "plus_one_neighbour_only_when_strictly_closer", "ring_loop_bound_times_enable_icp",
                    "point_loop_strides_by_icp_skip_from_zero", "ring_counts_when_search_found_something",
                    "degenerate_planes_skipped_by_icp_norm_condition") == {}


def test_the_solve_runs_on_ceres_defaults_except_the_linear_solver():
    opts = _facts()["solver_options"]
    assert opts == {"linear_solver_type": "ceres::DENSE_SCHUR", "minimizer_progress_to_stdout": "false"}, opts
    P = ol.default_params()                                                      # what the oracle (and the library) take for "defaults"
    assert (P.max_num_iterations, P.function_tolerance, P.gradient_tolerance, P.parameter_tolerance) == (50, 1e-6, 1e-10, 1e-8)
    assert (P.initial_trust_region_radius, P.min_relative_decrease, P.min_lm_diagonal, P.max_lm_diagonal) == (1e4, 1e-3, 1e-6, 1e32)


def test_rounding_points_of_utility_h_as_written():
    """utility.h:35-39,51-53,97-103: where the reference computes in float and where in double -- the oracle's sub_norm2 and
    transform_point restate exactly these lines (and the HIP kernels follow the oracle bit for bit)."""
    # subtract_assign: component-wise float subtraction IN PLACE on a pcl::PointXYZ (float members)
    # norm2: the FLOAT expression x*x + y*y + z*z, widened to double only by the return type
    # transform_point: widen to double, rotate in double, add the translation in double, store back to the float members
    assert _written("subtract_assign_componentwise_float_in_place", "norm2_float_expression_returned_as_double",
                    "transform_point_rotates_and_adds_in_double_stores_float") == {}
    # the oracle does the same on a point where float and double arithmetic differ visibly
    p = np.array([1.0000001, 2.0000002, -3.0000005], dtype=np.float32)
    x = np.array([0.3, -0.2, 0.1, 1e-3, 2e-3, 3e-3])
    got = ol.transform_point(p, x)
    rot = ol.rotate_point(x[:3], p.astype(np.float64))
    want = (rot + x[3:]).astype(np.float32)
    assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # pose_mat2vec / pose_vec2mat: column-major R from Ceres, T(i, j) = R[j * 3 + i]
    assert _written("pose_conversions_column_major") == {}
    T = ol.pose_vec_to_mat(x)
    Rcol = np.stack([ol.rotate_point(x[:3], e) for e in np.eye(3)], axis=1)      # column j = R e_j
    assert np.allclose(T[:3, :3], Rcol, atol=1e-15) and np.allclose(T[:3, 3], x[3:])


def test_visual_gates_as_written():
    """velo.h:674-682,709,739-742,772-775: squared norm against thresh*reject/iter * thresh*reject/iter (evaluated left to right -- the
    oracle and the gate kernel multiply in that order), |r| against thresh*reject/iter for the epipolar block (written with `abs`,
    restated as fabs), `continue` on failure -- which also skips the match's remaining residual types; only from the second iteration on."""
    assert _written("visual_gate_3D3D_squared_norm_left_to_right_from_second_iteration", "visual_gate_3D2D_squared_norm_left_to_right_from_second_iteration",
                    "visual_gate_3D2D_threshold_shared_by_two_blocks", "visual_gate_2D2D_absolute_value") == {}
    # the left-to-right product differs from (thresh*reject/iter)^2 in the last bit for some thresholds: both restatements take the written order
    P = ol.default_params()
    a, b, it = P.loss_thresh_3D2D, P.outlier_reject, 2
    assert a * b / it * a * b / it == ((((a * b) / it) * a) * b) / it


def test_ring_segmenter_as_written():
    """kitti.h:164-183: a new ring where x > 0 and the sign of y flips (strict comparisons, prev_y starts at 0); rings re-ordered by
    _i - 1 - (i + _i/2) % _i -- what tests/segmenter_ref.py transcribes."""
    assert _written("segmenter_new_ring_where_x_positive_and_y_flips", "segmenter_ring_reorder_and_velo_to_cam") == {}


def test_widened_rows_as_written():
    """The lines the oracle's restatements of SURVEY 8(f) rows 3-4 follow: linterpolate in float (utility.h:7-29), the projection, window
    test and occlusion-stack rules of projectLidarToCamera (velo.h:345-366), the bisection and acceptance test of featureDepthAssociation
    (velo.h:397-422), the losses of triangulatePoint (velo.h:1078-1122)."""
    assert _written("linterpolate_in_float", "projection_and_window_test", "occlusion_stack_rules", "depth_association_bisection_and_acceptance",
                    "triangulation_losses") == {}


def test_residual_stats_as_written():
    """velo.h:921-1025: evaluated WITHOUT loss functions; one number per block (sqrt of the squared rows for 3D3D / 3D2D / 2D3D, `abs` for
    2D2D and for everything behind the visual residuals = 3DPD); sums in block order, then sort; printed: element size/2 and sum/size."""
    assert _written("residual_stats_without_loss", "residual_stats_block_norms", "residual_stats_sum_before_sort",
                    "residual_stats_median_and_mean_per_type") == {}
