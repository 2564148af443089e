"""ctypes mirror of include/velo_hip.h -- plumbing only, no arithmetic happens in Python.

The shared library (csrc/libvelo_hip.so, built by build.py / __graft_entry__.build()) is the product.
If it is missing or no MI355X is visible every entry point raises: there is NO CPU fallback and this
module never imports anything from oracle/.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libvelo_hip.so")

VELO_MAX_SOLVES = 64
RESIDUAL_NAMES = {0: "3D3D", 1: "3D2D", 2: "2D3D", 3: "2D2D"}
TERMINATION_NAMES = {0: "CONVERGENCE", 1: "NO_CONVERGENCE", 2: "FAILURE"}


class VeloError(RuntimeError):
    pass


class VeloParams(C.Structure):
    _fields_ = [
        ("icp_skip", C.c_int32), ("f2f_iterations", C.c_int32), ("icp_iterations", C.c_int32),
        ("enable_icp", C.c_int32), ("enable_2d2d", C.c_int32), ("enable_3d2d", C.c_int32),
        ("max_num_iterations", C.c_int32), ("max_consecutive_invalid_steps", C.c_int32),
        ("weight_3D2D", C.c_double), ("weight_2D2D", C.c_double), ("weight_3DPD", C.c_double),
        ("loss_thresh_3D2D", C.c_double), ("loss_thresh_2D2D", C.c_double),
        ("loss_thresh_3DPD", C.c_double), ("loss_thresh_3D3D", C.c_double),
        ("outlier_reject", C.c_double), ("correspondence_thresh_icp", C.c_double),
        ("icp_norm_condition", C.c_double),
        ("function_tolerance", C.c_double), ("gradient_tolerance", C.c_double),
        ("parameter_tolerance", C.c_double), ("initial_trust_region_radius", C.c_double),
        ("max_trust_region_radius", C.c_double), ("min_trust_region_radius", C.c_double),
        ("min_relative_decrease", C.c_double), ("min_lm_diagonal", C.c_double),
        ("max_lm_diagonal", C.c_double),
    ]


class VeloSolveSummary(C.Structure):
    _fields_ = [
        ("termination", C.c_int32), ("lm_iterations", C.c_int32), ("evaluations", C.c_int32),
        ("n_icp_valid", C.c_int32), ("n_visual_blocks", C.c_int32), ("n_visual_residuals", C.c_int32),
        ("initial_cost", C.c_double), ("final_cost", C.c_double),
    ]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class VeloScanRef(C.Structure):
    _fields_ = [("xyz", C.c_void_p), ("stride_bytes", C.c_int64), ("ring_offsets", C.c_void_p), ("n_rings", C.c_int32),
                ("on_device", C.c_int32)]


VELO_MAX_STATS = 4
RESIDUAL_TYPE_NAMES = ("3D3D", "3D2D", "2D3D", "2D2D", "3DPD")


class VeloDescJob(C.Structure):
    """velo_desc_job: one (query, train) pair of 64-byte descriptor sets"""
    _fields_ = [("query", C.c_void_p), ("n_query", C.c_int32), ("train", C.c_void_p), ("n_train", C.c_int32)]


class VeloTrackJob(C.Structure):
    """velo_track_job: n points tracked from the previous image of prev_cam into the current image of cam"""
    _fields_ = [("prev_cam", C.c_int32), ("cam", C.c_int32), ("prev_xy", C.c_void_p), ("n", C.c_int32)]


class VeloLkParams(C.Structure):
    """velo_lk_params: calcOpticalFlowPyrLK's window, levels and termination as trackFeatures uses them (kitti.h:5-6,17; velo.h:60-67)"""
    _fields_ = [("window", C.c_int32), ("max_level", C.c_int32), ("max_count", C.c_int32), ("reserved", C.c_int32),
                ("epsilon", C.c_double), ("min_eig_threshold", C.c_double), ("flow_outlier", C.c_double)]


def lk_params(window: int = 21, max_level: int = 4, max_count: int = 30, epsilon: float = 0.01, min_eig_threshold: float = 1e-4,
              flow_outlier: float = 20000.0) -> VeloLkParams:
    return VeloLkParams(int(window), int(max_level), int(max_count), 0, float(epsilon), float(min_eig_threshold), float(flow_outlier))


IMAGE_KINDS = {"img": 0, "dx": 1, "dy": 2}


class VeloDetectJob(C.Structure):
    """velo_detect_job: corners of the current image of cam, flagged against n_existing points of the frame"""
    _fields_ = [("cam", C.c_int32), ("n_existing", C.c_int32), ("existing_xy", C.c_void_p)]


class VeloGfttParams(C.Structure):
    """velo_gftt_params: cv::GFTTDetector's arguments as detectFeatures uses them (main.cpp:84-87; kitti.h:7,18,19)"""
    _fields_ = [("max_corners", C.c_int32), ("block_size", C.c_int32), ("quality_level", C.c_double), ("min_distance", C.c_double)]


def gftt_params(max_corners: int = 3000, quality_level: float = 0.001, min_distance: float = 12.0, block_size: int = 3) -> VeloGfttParams:
    return VeloGfttParams(int(max_corners), int(block_size), float(quality_level), float(min_distance))


class VeloFrameCam(C.Structure):
    """velo_frame_cam: one camera of a frame for velo_frames_put_frame -- ids, canonical keypoints, optional FREAK rows, the window"""
    _fields_ = [("ids", C.c_void_p), ("keypoints_xy", C.c_void_p), ("rows", C.c_void_p), ("n", C.c_int32), ("bounds", C.c_double * 4)]


VELO_PUT_OBSERVE = 1


class FrameCam:
    """One camera of a frame as frames_put_frame takes it: ids [n], keypoints_xy [n, 2] (canonical), window (min_x, max_x, min_y,
    max_y: project_lidar's) and optionally the FREAK rows, uint8 [n, 64].  Holds contiguous copies for the duration of the call."""

    def __init__(self, ids, keypoints_xy, window, rows=None):
        self.ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
        self.keypoints_xy = np.ascontiguousarray(np.asarray(keypoints_xy, dtype=np.float32).reshape(-1, 2))
        if len(self.ids) != len(self.keypoints_xy):
            raise ValueError("FrameCam: one keypoint per id")
        self.window = _dvec(window, 4)
        self.rows = None
        if rows is not None:
            r = np.ascontiguousarray(np.asarray(rows, dtype=np.uint8))
            r = r.reshape(0, 64) if r.size == 0 else r
            if r.ndim != 2 or r.shape[1] != 64 or len(r) != len(self.ids):
                raise ValueError(f"FrameCam: descriptors must be uint8 (n, 64) with one row per id, got shape {r.shape}")
            self.rows = r

    def as_struct(self) -> VeloFrameCam:
        n = len(self.ids)
        rows = None
        if self.rows is not None:                     # an empty row set is still "rows given": any non-null address says so
            rows = self.rows.ctypes.data if n else self.window.ctypes.data
        return VeloFrameCam(self.ids.ctypes.data if n else None, self.keypoints_xy.ctypes.data if n else None, rows, n,
                            (C.c_double * 4)(*self.window))


class VeloBaParams(C.Structure):
    _fields_ = [("weight_3d", C.c_double), ("reserved", C.c_int32 * 2)]


class VeloBaIteration(C.Structure):
    _fields_ = [("status", C.c_int32), ("iteration", C.c_int32), ("cost", C.c_double), ("candidate_cost", C.c_double),
                ("radius", C.c_double), ("model_change", C.c_double), ("step_norm", C.c_double)]


BA_MAX_FREE, BA_MAX_TRACE = 10, 50
BA_ACCEPTED, BA_REJECTED, BA_INVALID, BA_PARAMETER, BA_FUNCTION, BA_GRADIENT = range(6)


class VeloBaSummary(C.Structure):
    _fields_ = [("termination", C.c_int32), ("iterations", C.c_int32), ("evaluations", C.c_int32), ("n_landmarks", C.c_int32),
                ("n_blocks", C.c_int32), ("n_residuals", C.c_int32), ("n_trace", C.c_int32), ("reserved", C.c_int32),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("trace", VeloBaIteration * BA_MAX_TRACE)]


class VeloGraphParams(C.Structure):
    _fields_ = [("cg_tolerance", C.c_double), ("cg_max_iterations", C.c_int32), ("reserved", C.c_int32 * 5)]


class VeloGraphIteration(C.Structure):
    _fields_ = [("status", C.c_int32), ("iteration", C.c_int32), ("cost", C.c_double), ("candidate_cost", C.c_double),
                ("radius", C.c_double), ("model_change", C.c_double), ("step_norm", C.c_double), ("cg_iterations", C.c_int32),
                ("reserved", C.c_int32), ("cg_residual", C.c_double)]


GRAPH_MAX_TRACE = 50
GRAPH_SOLVER_CG, GRAPH_SOLVER_ENVELOPE = 0, 1          # velo_graph_params.reserved[0]
GRAPH_SOLVERS = {"cg": GRAPH_SOLVER_CG, "envelope": GRAPH_SOLVER_ENVELOPE}
GRAPH_DEFAULT_MAX_WORK = 1 << 24                       # velo_graph_params.reserved[1] == 0


class VeloGraphSummary(C.Structure):
    _fields_ = [("termination", C.c_int32), ("iterations", C.c_int32), ("evaluations", C.c_int32), ("n_nodes", C.c_int32),
                ("n_free", C.c_int32), ("n_edges", C.c_int32), ("n_trace", C.c_int32), ("reserved", C.c_int32),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("trace", VeloGraphIteration * GRAPH_MAX_TRACE)]


class VeloResidualStat(C.Structure):
    _fields_ = [("median", C.c_double), ("mean", C.c_double), ("count", C.c_int64)]


class VeloResidualStats(C.Structure):
    """residualStats (velo.h:921-1025): per residual type median / mean / count of the block norms, loss not applied."""
    _fields_ = [("type", VeloResidualStat * 5), ("cost", C.c_double), ("n_blocks", C.c_int32), ("n_residuals", C.c_int32)]

    def as_dict(self):
        d = {n: dict(median=self.type[k].median, mean=self.type[k].mean, count=self.type[k].count) for k, n in enumerate(RESIDUAL_TYPE_NAMES)}
        d.update(cost=self.cost, n_blocks=self.n_blocks, n_residuals=self.n_residuals)
        return d


class VeloSummary(C.Structure):
    _fields_ = [
        ("n_solves", C.c_int32), ("n_assoc_rounds", C.c_int32), ("n_queries", C.c_int32),
        ("n_target", C.c_int32),
        ("algorithmic_bytes", C.c_uint64), ("assoc_bytes", C.c_uint64),
        ("assoc_kernel_ms", C.c_double), ("assoc_kernel_launches", C.c_int32),
        ("eval_kernel_launches", C.c_int32), ("eval_kernel_ms", C.c_double),
        ("solves", VeloSolveSummary * VELO_MAX_SOLVES),
        ("n_residual_stats", C.c_int32), ("reserved", C.c_int32),
        ("residual_stats", VeloResidualStats * VELO_MAX_STATS),
    ]

    def as_dict(self):
        d = {k: getattr(self, k) for k, _ in self._fields_ if k not in ("solves", "residual_stats", "reserved")}
        d["solves"] = [self.solves[i].as_dict() for i in range(min(self.n_solves, VELO_MAX_SOLVES))]
        d["residual_stats"] = [self.residual_stats[i].as_dict() for i in range(min(self.n_residual_stats, VELO_MAX_STATS))]
        return d


MATCH_DTYPE = np.dtype([
    ("p3_1", np.float32, 3), ("p3_2", np.float32, 3), ("p2_1", np.float32, 2), ("p2_2", np.float32, 2),
    ("t_cam", np.float32, 3), ("cam", np.int32), ("point1", np.int32), ("point2", np.int32),
    ("d1", np.uint8), ("d2", np.uint8), ("pad", np.uint8, 2)], align=True)
GOOD_DTYPE = np.dtype([("cam", np.int32), ("point1", np.int32), ("point2", np.int32),
                       ("residual_type", np.int32)], align=True)
CORR_DTYPE = np.dtype([
    ("valid", np.int32), ("ring_i", np.int32), ("idx_i", np.int32), ("ring_j", np.int32),
    ("idx_j", np.int32), ("idx_k", np.int32), ("src_ring", np.int32), ("src_idx", np.int32),
    ("dist_i", np.float32), ("dist_j", np.float32),
    ("p", np.float32, 3), ("n", np.float32, 3), ("v0", np.float32, 3)], align=True)
PARTIAL_DTYPE = np.dtype([
    ("key1", np.uint64), ("key2", np.uint64), ("ring1", np.int32), ("ring2", np.int32), ("idx1", np.int32),
    ("idx_k", np.int32), ("idx2", np.int32), ("pad", np.int32), ("v0", np.float32, 3), ("v2", np.float32, 3),
    ("v1", np.float32, 3), ("pad2", np.float32)], align=True)
TRI_OBS_DTYPE = np.dtype([("kind", np.int32), ("frame", np.int32), ("cam", np.int32), ("s", np.float32, 3)])
TRI_RESULT_DTYPE = np.dtype([("n_solves", np.int32), ("termination", np.int32), ("lm_iterations", np.int32),
                             ("evaluations", np.int32), ("final_cost", np.float64)])
TRI_OBS_3D, TRI_OBS_2D = 0, 1
FUNCTOR_DTYPE = np.dtype([("kind", np.int32), ("reserved", np.int32), ("c", np.float64, 9)])
FUNCTOR_3DPD = 4
assert MATCH_DTYPE.itemsize == 68 and GOOD_DTYPE.itemsize == 16 and CORR_DTYPE.itemsize == 76 and PARTIAL_DTYPE.itemsize == 80
assert TRI_OBS_DTYPE.itemsize == 24 and TRI_RESULT_DTYPE.itemsize == 24 and FUNCTOR_DTYPE.itemsize == 80


KERNEL_TIME_DTYPE = np.dtype([("name", "S48"), ("ms", "<f8"), ("launches", "<i8"), ("sampled", "<i8"), ("algorithmic_bytes", "<u8")])
assert KERNEL_TIME_DTYPE.itemsize == 80


def matches_from_dict(rec: dict) -> np.ndarray:
    """synth.stereo_matches() dict -> packed velo_match array."""
    n = len(rec["cam"])
    m = np.zeros(n, dtype=MATCH_DTYPE)
    for k in ("p3_1", "p3_2", "p2_1", "p2_2", "t_cam", "cam", "point1", "point2", "d1", "d2"):
        m[k] = rec[k]
    return m


def pack_triangulation(camera_poses, cam_trans, obs, obs_offsets, points_xyz, initial_guess):
    """Contiguous, typed copies of the arguments of velo_triangulate_points (shared with the test-side oracle wrapper)."""
    poses = np.ascontiguousarray(np.asarray(camera_poses, dtype=np.float64).reshape(-1, 6))
    ct = np.ascontiguousarray(np.asarray(cam_trans, dtype=np.float32).reshape(-1, 3))
    ob = np.ascontiguousarray(obs, dtype=TRI_OBS_DTYPE)
    off = np.ascontiguousarray(obs_offsets, dtype=np.int32)
    pts = np.array(np.asarray(points_xyz, dtype=np.float32).reshape(-1, 3), copy=True, order="C")
    if len(off) - 1 != len(pts):
        raise ValueError("obs_offsets must have one more entry than there are landmarks")
    init = None if initial_guess is None else np.ascontiguousarray(np.asarray(initial_guess).astype(np.uint8))
    if init is not None and len(init) != len(pts):
        raise ValueError("initial_guess: one flag per landmark")
    return poses, ct, ob, off, pts, init


def default_params() -> VeloParams:
    """The reference's constants (kitti.h:8-10,20-32; main.cpp:43-45) + Ceres defaults, filled in Python so
    that it also works on a box without the library; tests check it against velo_default_params()."""
    p = VeloParams()
    p.icp_skip, p.f2f_iterations, p.icp_iterations = 200, 2, 3
    p.enable_icp = p.enable_2d2d = p.enable_3d2d = 1
    p.max_num_iterations, p.max_consecutive_invalid_steps = 50, 5
    p.weight_3D2D, p.weight_2D2D, p.weight_3DPD = 10.0, 500.0, 1.0
    p.loss_thresh_3D2D, p.loss_thresh_2D2D, p.loss_thresh_3DPD, p.loss_thresh_3D3D = 0.01, 0.00002, 0.1, 0.04
    p.outlier_reject, p.correspondence_thresh_icp, p.icp_norm_condition = 5.0, 0.5, 1e-5
    p.function_tolerance, p.gradient_tolerance, p.parameter_tolerance = 1e-6, 1e-10, 1e-8
    p.initial_trust_region_radius, p.max_trust_region_radius, p.min_trust_region_radius = 1e4, 1e16, 1e-32
    p.min_relative_decrease, p.min_lm_diagonal, p.max_lm_diagonal = 1e-3, 1e-6, 1e32
    return p


# ---- every symbol include/velo_hip.h declares (tests check the .so exports all of them) -----------
_P = C.POINTER
_ctx = C.c_void_p
_dp = _P(C.c_double)
SIGNATURES = {
    "velo_create": (C.c_int, [_P(_ctx), C.c_int]),
    "velo_destroy": (C.c_int, [_ctx]),
    "velo_last_error": (C.c_char_p, []),
    "velo_version": (C.c_char_p, []),
    "velo_default_params": (C.c_int, [_P(VeloParams)]),
    "velo_set_params": (C.c_int, [_ctx, _P(VeloParams)]),
    "velo_get_params": (C.c_int, [_ctx, _P(VeloParams)]),
    "velo_set_timing": (C.c_int, [_ctx, C.c_int]),
    "velo_get_kernel_times": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.POINTER(C.c_int32), C.c_int32]),
    "velo_set_target": (C.c_int, [_ctx, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int]),
    "velo_set_target_part": (C.c_int, [_ctx, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int]),
    "velo_set_source": (C.c_int, [_ctx, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_int]),
    "velo_set_scan_velodyne": (C.c_int, [_ctx, C.c_int32, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int]),
    "velo_source_to_target": (C.c_int, [_ctx]),
    "velo_share_target": (C.c_int, [_ctx, _ctx]),
    "velo_cache_create": (C.c_int, [_P(C.c_void_p), C.c_int32, C.c_int32]),
    "velo_cache_destroy": (C.c_int, [C.c_void_p]),
    "velo_cache_store": (C.c_int, [C.c_void_p, C.c_int32, _ctx, C.c_int32]),
    "velo_cache_load": (C.c_int, [C.c_void_p, C.c_int32, _ctx, C.c_int32]),
    "velo_cache_contains": (C.c_int, [C.c_void_p, C.c_int32]),
    "velo_cache_frames": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_int32]),
    "velo_get_ring_offsets": (C.c_int, [_ctx, C.c_int32, C.c_void_p, C.c_int32, _P(C.c_int32)]),
    "velo_get_cloud": (C.c_int, [_ctx, C.c_int32, C.c_void_p, C.c_int32, _P(C.c_int32)]),
    "velo_set_visual": (C.c_int, [_ctx, C.c_void_p, C.c_int32]),
    "velo_associate": (C.c_int, [_ctx, _dp, C.c_int32, _P(C.c_int32)]),
    "velo_associate_partial": (C.c_int, [_ctx, _dp, C.c_int32]),
    "velo_get_partials": (C.c_int, [_ctx, C.c_void_p, C.c_int32, _P(C.c_int32)]),
    "velo_merge_partials": (C.c_int, [_ctx, _P(C.c_void_p), C.c_int32, _P(C.c_int32)]),
    "velo_get_correspondences": (C.c_int, [_ctx, C.c_void_p, C.c_int32, _P(C.c_int32)]),
    "velo_build_visual": (C.c_int, [_ctx, _dp, C.c_int32, _P(C.c_int32)]),
    "velo_get_good_matches": (C.c_int, [_ctx, C.c_void_p, C.c_int32, _P(C.c_int32)]),
    "velo_evaluate": (C.c_int, [_ctx, _dp, _dp, _dp, _dp]),
    "velo_evaluate_rows": (C.c_int, [_ctx, _dp, _dp, _dp, C.c_int32, _P(C.c_int32)]),
    "velo_evaluate_functors": (C.c_int, [_ctx, C.c_void_p, C.c_int32, _dp, _dp, _dp]),
    "velo_solve": (C.c_int, [_ctx, _dp, _P(VeloSolveSummary)]),
    "velo_frame_to_frame": (C.c_int, [_ctx, _dp, _dp, _P(VeloSummary)]),
    "velo_frame_to_frame_batch": (C.c_int, [_P(_ctx), C.c_int32, _dp, _dp, _P(VeloSummary)]),
    "velo_register_batch": (C.c_int, [_P(_ctx), C.c_int32, C.c_void_p, C.c_void_p, _dp, _dp, _P(VeloSummary)]),
    "velo_register_batch_visual": (C.c_int, [_P(_ctx), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, _dp, _dp, _P(VeloSummary)]),
    "velo_hint_next_source": (C.c_int, [_ctx, C.c_void_p]),
    "velo_hint_next_frame": (C.c_int, [_ctx, C.c_void_p]),
    "velo_register_sequences": (C.c_int, [_P(_ctx), C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, _dp, _dp, _dp, _dp, _P(VeloSummary), C.c_int32]),
    "velo_pose_vec_to_mat": (C.c_int, [_dp, _dp]),
    "velo_pose_mat_to_vec": (C.c_int, [_dp, _dp]),
    "velo_pose_handoff": (C.c_int, [C.c_int32, _dp, _dp, _dp]),
    "velo_comm_unique_id": (C.c_int, [C.c_char_p]),
    "velo_comm_init": (C.c_int, [_ctx, C.c_char_p, C.c_int32, C.c_int32]),
    "velo_comm_destroy": (C.c_int, [_ctx]),
    "velo_comm_peer_export": (C.c_int, [_ctx, C.c_char_p]),
    "velo_comm_peer_attach": (C.c_int, [_ctx, C.c_char_p, C.c_int32, C.c_int32]),
    "velo_comm_info": (C.c_int, [_ctx, _P(C.c_int32), _P(C.c_int32), _P(C.c_int32)]),
    "velo_chain_stats": (C.c_int, [_ctx, _P(C.c_int32), _P(C.c_int32)]),
    "velo_set_residual_stats": (C.c_int, [_ctx, C.c_int]),
    "velo_residual_stats_at": (C.c_int, [_ctx, _P(C.c_double), _P(VeloResidualStats)]),
    "velo_comm_peer_export_records": (C.c_int, [_ctx, C.c_int32, C.c_char_p]),
    "velo_comm_peer_attach_records": (C.c_int, [_ctx, C.c_char_p, C.c_int32]),
    "velo_comm_set_target_sharded": (C.c_int, [_ctx, C.c_int]),
    "velo_set_query_shard": (C.c_int, [_ctx, C.c_int32, C.c_int32]),
    "velo_synchronize": (C.c_int, [_ctx]),
    "velo_project_lidar": (C.c_int, [_ctx, C.c_int32, C.c_void_p, _dp, _P(C.c_int32)]),
    "velo_get_projection": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, _P(C.c_int32)]),
    "velo_depth_association": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_int32, C.c_void_p, _P(C.c_int32)]),
    "velo_triangulate_points": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "velo_match_descriptors": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p]),
    "velo_set_images": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "velo_get_image_level": (C.c_int, [_ctx, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int64, C.c_void_p]),
    "velo_track_features": (C.c_int, [_ctx, C.c_void_p, C.c_int32, _P(VeloLkParams), C.c_void_p, C.c_void_p, C.c_void_p]),
    "velo_default_gftt_params": (C.c_int, [_P(VeloGfttParams)]),
    "velo_detect_features": (C.c_int, [_ctx, C.c_void_p, C.c_int32, _P(VeloGfttParams), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "velo_get_corner_response": (C.c_int, [_ctx, C.c_int32, C.c_void_p, C.c_int64]),
    "velo_set_images_batch": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p]),
    "velo_track_features_batch": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, _P(VeloLkParams), C.c_void_p,
                                            C.c_void_p, C.c_void_p]),
    "velo_detect_features_batch": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, _P(VeloGfttParams), C.c_int32,
                                             C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "velo_landmarks_reset": (C.c_int, [_ctx, C.c_int32, C.c_void_p, C.c_int32]),
    "velo_landmarks_set_pose": (C.c_int, [_ctx, C.c_int32, _dp]),
    "velo_landmarks_observe": (C.c_int, [_ctx, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "velo_landmarks_triangulate": (C.c_int, [_ctx, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, _P(C.c_int32)]),
    "velo_landmarks_triangulate_batch": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                                   C.c_void_p]),
    "velo_landmarks_at_frame": (C.c_int, [_ctx, C.c_int32, _dp, C.c_void_p, C.c_void_p, C.c_int32, _P(C.c_int32)]),
    "velo_landmarks_get": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "velo_landmarks_frame_count": (C.c_int, [_ctx, C.c_int32, _P(C.c_int32), _P(C.c_int32)]),
    "velo_landmarks_info": (C.c_int, [_ctx, C.c_void_p]),
    "velo_default_ba_params": (C.c_int, [_P(VeloBaParams)]),
    "velo_landmarks_adjust": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, _P(VeloBaParams), C.c_void_p, _P(VeloBaSummary)]),
    "velo_landmarks_adjust_system": (C.c_int, [_ctx, C.c_void_p, C.c_int32, C.c_int32, _P(VeloBaParams), _dp, C.c_void_p, C.c_void_p]),
    "velo_default_graph_params": (C.c_int, [_P(VeloGraphParams)]),
    "velo_graph_reset": (C.c_int, [_ctx, C.c_int32]),
    "velo_graph_set_pose": (C.c_int, [_ctx, C.c_int32, _dp]),
    "velo_graph_set_poses": (C.c_int, [_ctx, C.c_int32, C.c_int32, C.c_void_p]),
    "velo_graph_add_edges": (C.c_int, [_ctx, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "velo_graph_add_edges_weighted": (C.c_int, [_ctx, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "velo_graph_edge_stats": (C.c_int, [_ctx, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]),
    "velo_graph_edge_information": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p]),
    "velo_graph_optimize": (C.c_int, [_ctx, C.c_void_p, C.c_int32, _P(VeloGraphParams), _P(VeloGraphSummary)]),
    "velo_graph_get_poses": (C.c_int, [_ctx, C.c_int32, C.c_int32, C.c_void_p]),
    "velo_graph_info": (C.c_int, [_ctx, C.c_void_p]),
    "velo_graph_order": (C.c_int, [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "velo_graph_order_extend": (C.c_int, [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "velo_graph_system": (C.c_int, [_ctx, C.c_void_p, C.c_int32, _dp, C.c_void_p, C.c_void_p]),
    "velo_graph_retain": (C.c_int, [_ctx, C.c_void_p, C.c_int32, _P(VeloGraphParams), C.c_void_p, C.c_int32]),
    "velo_graph_release": (C.c_int, [_ctx]),
    "velo_graph_retained": (C.c_int, [_ctx, C.c_void_p, C.c_void_p, C.c_int32]),
    "velo_graph_covariance": (C.c_int, [_ctx, C.c_void_p, C.c_int32, _P(VeloGraphParams), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]),
    "velo_graph_edge_gate": (C.c_int, [_ctx, C.c_void_p, C.c_int32, _P(VeloGraphParams), C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "velo_graph_loop_candidates": (C.c_int, [_ctx, C.c_void_p, C.c_int32, _P(VeloGraphParams), C.c_int32, C.c_int32, C.c_double, C.c_double, C.c_int32,
                                             C.c_void_p, C.c_void_p, C.c_void_p, _P(C.c_int32)]),
    "velo_frames_reset": (C.c_int, [_ctx, C.c_int32, C.c_void_p, C.c_int32]),
    "velo_frames_put": (C.c_int, [_ctx, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]),
    "velo_frames_drop": (C.c_int, [_ctx, C.c_int32]),
    "velo_frames_count": (C.c_int, [_ctx, C.c_int32, C.c_void_p, _P(C.c_int32)]),
    "velo_frames_info": (C.c_int, [_ctx, C.c_void_p]),
    "velo_build_matches": (C.c_int, [_ctx, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, _P(C.c_int32)]),
    "velo_build_matches_batch": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32,
                                           C.c_void_p]),
    "velo_get_visual": (C.c_int, [_ctx, C.c_void_p, C.c_int32, _P(C.c_int32)]),
    "velo_frames_get": (C.c_int, [_ctx, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32,
                                  _P(C.c_int32), _P(C.c_int32), _P(C.c_int32)]),
    "velo_frames_keep": (C.c_int, [_ctx, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, _P(C.c_int32), _P(C.c_int32)]),
    "velo_frames_prune": (C.c_int, [_ctx, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, _P(C.c_int32)]),
    "velo_frames_prune_batch": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]),
    "velo_frames_put_descriptors": (C.c_int, [_ctx, C.c_int32, C.c_int32, C.c_void_p, C.c_int32]),
    "velo_frames_desc_info": (C.c_int, [_ctx, C.c_void_p]),
    "velo_build_matches_desc": (C.c_int, [_ctx, C.c_int32, C.c_int32, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_int32, _P(C.c_int32)]),
    "velo_build_matches_desc_batch": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p,
                                                C.c_int32, C.c_void_p]),
    "velo_match_frames": (C.c_int, [_ctx, C.c_int32, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p]),
    "velo_frames_put_frame": (C.c_int, [_ctx, C.c_int32, C.c_int32, C.c_void_p, C.c_double, C.c_int32, C.c_void_p]),
    "velo_frames_put_frame_batch": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_int32, C.c_void_p]),
    "velo_map_create": (C.c_int, [_P(C.c_void_p), C.c_int32, C.c_int32, C.c_int64]),
    "velo_map_destroy": (C.c_int, [C.c_void_p]),
    "velo_map_insert": (C.c_int, [C.c_void_p, _ctx, C.c_int32, C.c_int32, _dp, _P(C.c_int32)]),
    "velo_map_set_pose": (C.c_int, [C.c_void_p, C.c_int32, _dp]),
    "velo_map_drop": (C.c_int, [C.c_void_p, C.c_int32]),
    "velo_map_clear": (C.c_int, [C.c_void_p]),
    "velo_map_frames": (C.c_int, [C.c_void_p, _P(C.c_int32), C.c_int32]),
    "velo_map_info": (C.c_int, [C.c_void_p, _P(C.c_int64)]),
    "velo_map_get_scan": (C.c_int, [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, _P(C.c_int32), C.c_void_p, C.c_int32, _P(C.c_int32), _dp]),
    "velo_map_load": (C.c_int, [C.c_void_p, _ctx, _dp]),
    "velo_map_load_batch": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int32, _dp]),
}

_lib = None
_libs_by_path = {}
LIB_PATH_DIAG = os.path.join(os.path.dirname(LIB_PATH), "libvelo_hip_diag.so")


def load_library(path: Optional[str] = None) -> C.CDLL:
    """dlopen the HIP library and type every entry point.  Raises VeloError when it has not been built.
    path: another build of the same source (the tools' / variant tests' diagnostics build, see load_diagnostics_library)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    if path is not None and path in _libs_by_path:
        return _libs_by_path[path]
    p = path or os.environ.get("VELO_LIB_PATH") or LIB_PATH      # VELO_LIB_PATH: A/B builds on one GPU box
    if not os.path.exists(p):
        raise VeloError(f"{p} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                        "(hipcc --offload-arch=gfx950). There is no CPU fallback.")
    lib = C.CDLL(p, mode=C.RTLD_GLOBAL)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError here = header/library drift; tests guard it
        fn.restype, fn.argtypes = res, args
    if path is None:
        _lib = lib
    else:
        _libs_by_path[path] = lib
    return lib


def load_diagnostics_library() -> C.CDLL:
    """The -DVELO_DIAGNOSTICS build of the same source (libvelo_hip_diag.so): the only build that honours the A/B environment switches
    (kernel variants, grid shapes, VELO_DEBUG_SKIP ...).  The product library reads five documented knobs and ignores the rest, so the
    parity tests that sweep variants, and the dev tools, create their contexts on this one: Context(device, lib=load_diagnostics_library())."""
    return load_library(LIB_PATH_DIAG)


def _dvec(a, n):
    arr = np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(-1))
    if arr.size != n:
        raise ValueError(f"expected {n} doubles, got {arr.size}")
    return arr


def _ptr(arr: np.ndarray):
    return arr.ctypes.data_as(_dp)


class Context:
    """One scan-matching context = one `velo_ctx*` (device buffers + a HIP stream on `device`)."""

    def __init__(self, device: int = 0, lib: Optional[C.CDLL] = None, **params):
        self._lib = lib if lib is not None else load_library()
        self._h = _ctx()
        self._device = int(device)
        self._check(self._lib.velo_create(C.byref(self._h), int(device)))
        if params:
            self.set_params(**params)

    # -- helpers ---------------------------------------------------------------------------------
    def _check(self, status: int):
        if status != 0:
            msg = self._lib.velo_last_error()
            raise VeloError(f"velo status {status}: {msg.decode() if msg else ''}")

    def close(self):
        if getattr(self, "_h", None) and self._h.value:
            self._lib.velo_destroy(self._h)
            self._h = _ctx()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def handle(self):
        return self._h

    # -- configuration -------------------------------------------------------------------------------
    def get_params(self) -> VeloParams:
        p = VeloParams()
        self._check(self._lib.velo_get_params(self._h, C.byref(p)))
        return p

    def set_params(self, **kw):
        p = self.get_params()
        for k, v in kw.items():
            if not hasattr(p, k):
                raise AttributeError(f"velo_params has no field {k}")
            setattr(p, k, v)
        self._check(self._lib.velo_set_params(self._h, C.byref(p)))

    def set_timing(self, enable):
        """0 / False: off; 1 / True: association launches into the summary; 2: launches counted by kernel name, every 8th bracketed
        (kernel_times); 3: every launch bracketed."""
        self._check(self._lib.velo_set_timing(self._h, int(enable)))

    def kernel_times(self, reset: bool = True):
        """{kernel name: (ms, launches, algorithmic bytes)} accumulated since the last reset (velo_set_timing(ctx, 2))."""
        n = C.c_int32(0)
        self._check(self._lib.velo_get_kernel_times(self._h, None, 0, C.byref(n), 0))
        out = np.zeros(max(n.value, 1), dtype=KERNEL_TIME_DTYPE)
        self._check(self._lib.velo_get_kernel_times(self._h, C.c_void_p(out.ctypes.data), n.value, C.byref(n), int(bool(reset))))
        return {bytes(r["name"]).split(b"\0")[0].decode(): (float(r["ms"]), int(r["launches"]), int(r["algorithmic_bytes"])) for r in out[:n.value]}

    # -- inputs ----------------------------------------------------------------------------------------
    @staticmethod
    def _device_tensor_args(t, device, cols=(3, 4), what="xyz"):
        """A torch tensor handed over as a device pointer (on_device = 1): checked here because the library only sees an address.
        The library reads it on the context's own stream, so everything torch has queued that produces the tensor must be
        complete first (include/velo_hip.h, "device pointers"): the producing torch stream is synchronised before the call."""
        import torch
        if not t.is_cuda:
            raise ValueError(f"{what}: a torch tensor must live on the GPU (pass a numpy array for host data)")
        if t.dtype != torch.float32:
            raise ValueError(f"{what}: device tensor must be float32, got {t.dtype}")
        if t.dim() != 2 or t.shape[1] not in cols:
            raise ValueError(f"{what}: device tensor must be (n, {' or '.join(str(c) for c in cols)}), got {tuple(t.shape)}")
        if t.shape[0] > 1 and (t.stride(1) != 1 or t.stride(0) < 3):
            raise ValueError(f"{what}: the coordinates of a point must be contiguous (stride(1) == 1), got strides {t.stride()}")
        if device is not None and t.device.index != int(device):
            raise ValueError(f"{what}: tensor is on cuda:{t.device.index}, the context on device {int(device)}")
        torch.cuda.current_stream(t.device).synchronize()
        stride = (t.stride(0) if t.shape[0] > 1 else t.shape[1]) * t.element_size()
        return C.c_void_p(t.data_ptr()), stride

    @staticmethod
    def _cloud_args(xyz, ring_offsets, device=None):
        off = np.ascontiguousarray(np.asarray(ring_offsets, dtype=np.int32))
        if hasattr(xyz, "data_ptr"):   # a torch tensor on the GPU: (n,3) or (n,4) float32, row stride in bytes
            ptr, stride = Context._device_tensor_args(xyz, device)
            if len(off) and int(off[-1]) > xyz.shape[0]:
                raise ValueError(f"ring_offsets end at {int(off[-1])} but the tensor holds {xyz.shape[0]} points")
            return ptr, stride, off, 1, xyz
        a = np.asarray(xyz, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] not in (3, 4):
            raise ValueError("xyz must be (n,3) or (n,4) float32")
        a = np.ascontiguousarray(a)
        if len(off) and int(off[-1]) > a.shape[0]:
            raise ValueError(f"ring_offsets end at {int(off[-1])} but the array holds {a.shape[0]} points")
        return C.c_void_p(a.ctypes.data), a.strides[0], off, 0, a

    def set_target(self, xyz, ring_offsets):
        ptr, stride, off, dev, keep = self._cloud_args(xyz, ring_offsets, self._device)
        self._check(self._lib.velo_set_target(self._h, ptr, stride, C.c_void_p(off.ctypes.data), len(off) - 1, dev))

    def set_target_part(self, xyz, ring_offsets, first_ring: int, first_point: int):
        """Target-sharded mode: this context holds only a block of whole rings (local offsets, [0] == 0)."""
        ptr, stride, off, dev, keep = self._cloud_args(xyz, ring_offsets, self._device)
        self._check(self._lib.velo_set_target_part(self._h, ptr, stride, C.c_void_p(off.ctypes.data), len(off) - 1,
                                                   int(first_ring), int(first_point), dev))

    def associate_partial(self, x, iter: int):
        xv = _dvec(x, 6)
        self._check(self._lib.velo_associate_partial(self._h, _ptr(xv), int(iter)))

    def partials(self) -> np.ndarray:
        n = C.c_int32(0)
        self._check(self._lib.velo_get_partials(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=PARTIAL_DTYPE)
        if n.value:
            self._check(self._lib.velo_get_partials(self._h, C.c_void_p(out.ctypes.data), n.value, C.byref(n)))
        return out

    def merge_partials(self, tables) -> int:
        tabs = [np.ascontiguousarray(t, dtype=PARTIAL_DTYPE) for t in tables]
        arr = (C.c_void_p * len(tabs))(*[t.ctypes.data for t in tabs])
        n = C.c_int32(0)
        self._check(self._lib.velo_merge_partials(self._h, arr, len(tabs), C.byref(n)))
        return n.value

    def comm_set_target_sharded(self, enable: bool):
        self._check(self._lib.velo_comm_set_target_sharded(self._h, int(bool(enable))))

    def set_source(self, xyz, ring_offsets):
        ptr, stride, off, dev, keep = self._cloud_args(xyz, ring_offsets, self._device)
        self._check(self._lib.velo_set_source(self._h, ptr, stride, C.c_void_p(off.ctypes.data), len(off) - 1, dev))

    def set_scan_velodyne(self, as_target: bool, records, velo_to_cam):
        """Raw Velodyne records (n,4) float32 in file order (or a torch tensor on the GPU) -> rings on the device."""
        M = np.ascontiguousarray(np.asarray(velo_to_cam, dtype=np.float32).reshape(4, 4))
        if hasattr(records, "data_ptr"):
            (ptr, stride), n, dev = self._device_tensor_args(records, self._device, cols=(3, 4), what="records"), records.shape[0], 1
        else:
            a = np.ascontiguousarray(np.asarray(records, dtype=np.float32))
            ptr, stride, n, dev = C.c_void_p(a.ctypes.data), a.strides[0], a.shape[0], 0
        self._check(self._lib.velo_set_scan_velodyne(self._h, int(bool(as_target)), ptr, stride, n, C.c_void_p(M.ctypes.data), dev))

    def ring_offsets(self, of_target: bool) -> np.ndarray:
        n = C.c_int32(0)
        self._check(self._lib.velo_get_ring_offsets(self._h, int(bool(of_target)), None, 0, C.byref(n)))
        out = np.zeros(n.value + 1, dtype=np.int32)
        self._check(self._lib.velo_get_ring_offsets(self._h, int(bool(of_target)), C.c_void_p(out.ctypes.data), len(out), C.byref(n)))
        return out

    def source_to_target(self):
        """The device-resident source scan becomes the target of the next registration (no upload, no second segmentation)."""
        self._check(self._lib.velo_source_to_target(self._h))

    def share_target(self, src: "Context"):
        """Take the target `src` holds (cloud + index) by reference: scan-to-map batches keep ONE map for all their contexts."""
        self._check(self._lib.velo_share_target(self._h, src.handle))

    def cloud(self, of_target: bool) -> np.ndarray:
        n = C.c_int32(0)
        self._check(self._lib.velo_get_cloud(self._h, int(bool(of_target)), None, 0, C.byref(n)))
        out = np.zeros((n.value, 3), dtype=np.float32)
        if n.value:
            self._check(self._lib.velo_get_cloud(self._h, int(bool(of_target)), C.c_void_p(out.ctypes.data), n.value, C.byref(n)))
        return out

    def set_visual(self, matches):
        if isinstance(matches, dict):
            matches = matches_from_dict(matches)
        m = np.ascontiguousarray(matches, dtype=MATCH_DTYPE) if matches is not None else np.zeros(0, MATCH_DTYPE)
        self._check(self._lib.velo_set_visual(self._h, C.c_void_p(m.ctypes.data) if len(m) else None, len(m)))

    # -- pieces ------------------------------------------------------------------------------------------
    def associate(self, x, iter: int) -> int:
        xv = _dvec(x, 6)
        n = C.c_int32(0)
        self._check(self._lib.velo_associate(self._h, _ptr(xv), int(iter), C.byref(n)))
        return n.value

    def correspondences(self) -> np.ndarray:
        n = C.c_int32(0)
        self._check(self._lib.velo_get_correspondences(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=CORR_DTYPE)
        if n.value:
            self._check(self._lib.velo_get_correspondences(self._h, C.c_void_p(out.ctypes.data), n.value, C.byref(n)))
        return out

    def build_visual(self, x, iter: int) -> int:
        xv = _dvec(x, 6)
        n = C.c_int32(0)
        self._check(self._lib.velo_build_visual(self._h, _ptr(xv), int(iter), C.byref(n)))
        return n.value

    def good_matches(self) -> np.ndarray:
        n = C.c_int32(0)
        self._check(self._lib.velo_get_good_matches(self._h, None, 0, C.byref(n)))
        out = np.zeros(n.value, dtype=GOOD_DTYPE)
        if n.value:
            self._check(self._lib.velo_get_good_matches(self._h, C.c_void_p(out.ctypes.data), n.value, C.byref(n)))
        return out

    def evaluate(self, x):
        xv = _dvec(x, 6)
        cost = C.c_double(0)
        H = np.zeros(36)
        g = np.zeros(6)
        self._check(self._lib.velo_evaluate(self._h, _ptr(xv), C.byref(cost), _ptr(H), _ptr(g)))
        return cost.value, H.reshape(6, 6), g

    def evaluate_rows(self, x):
        xv = _dvec(x, 6)
        n = C.c_int32(0)
        self._lib.velo_evaluate_rows(self._h, _ptr(xv), None, None, 0, C.byref(n))
        r = np.zeros(n.value)
        J = np.zeros((n.value, 6))
        if n.value:
            self._check(self._lib.velo_evaluate_rows(self._h, _ptr(xv), _ptr(r), _ptr(J), n.value, C.byref(n)))
        return r, J

    def evaluate_functors(self, kinds, consts, x, want_jacobian: bool = True):
        """Seam 2 by value: raw residuals [n,3] and autodiff-equal Jacobians [n,3,6] of n functors (kind 0..3 = ResidualType
        order, 4 = cost3DPD; consts [n,<=9] = constructor arguments in the reference's order) at pose x."""
        kinds = np.asarray(kinds, dtype=np.int32).reshape(-1)
        consts = np.asarray(consts, dtype=np.float64)
        consts = consts.reshape(len(kinds), consts.size // max(len(kinds), 1))
        rec = np.zeros(len(kinds), dtype=FUNCTOR_DTYPE)
        rec["kind"] = kinds
        rec["c"][:, :consts.shape[1]] = consts
        xv = _dvec(x, 6)
        r = np.zeros((len(kinds), 3))
        J = np.zeros((len(kinds), 3, 6)) if want_jacobian else None
        self._check(self._lib.velo_evaluate_functors(self._h, C.c_void_p(rec.ctypes.data), len(kinds), _ptr(xv), _ptr(r),
                                                     _ptr(J) if want_jacobian else None))
        return r, J

    def solve(self, x):
        xv = _dvec(x, 6).copy()
        s = VeloSolveSummary()
        self._check(self._lib.velo_solve(self._h, _ptr(xv), C.byref(s)))
        return xv, s

    # -- the path ------------------------------------------------------------------------------------------
    def frame_to_frame(self, x0):
        xv = _dvec(x0, 6).copy()
        T = np.zeros(16)
        s = VeloSummary()
        self._check(self._lib.velo_frame_to_frame(self._h, _ptr(xv), _ptr(T), C.byref(s)))
        return xv, T.reshape(4, 4), s

    def synchronize(self):
        self._check(self._lib.velo_synchronize(self._h))

    # -- camera projection of a scan + keypoint depth (velo.h:329-497) -------------------------------------------
    def project_lidar(self, of_target: bool, cam_t, window) -> int:
        """projectLidarToCamera for one camera on the rings held as source/target; returns the number of kept points."""
        t = np.ascontiguousarray(np.asarray(cam_t, dtype=np.float32).reshape(-1))
        if t.size != 3:
            raise ValueError("cam_t: 3 floats")
        w = _dvec(window, 4)
        n = C.c_int32(0)
        self._check(self._lib.velo_project_lidar(self._h, int(bool(of_target)), C.c_void_p(t.ctypes.data), _ptr(w), C.byref(n)))
        return n.value

    def projection(self):
        """(proj_xy [n,2] f32, points_xyz [n,3] f32, ring_offsets [Rs+1] i32) of the last project_lidar."""
        nr = C.c_int32(0)
        self._check(self._lib.velo_get_projection(self._h, None, None, 0, None, 0, C.byref(nr)))
        off = np.zeros(nr.value + 1, dtype=np.int32)
        self._check(self._lib.velo_get_projection(self._h, None, None, 0, C.c_void_p(off.ctypes.data), off.size, C.byref(nr)))
        n = int(off[-1])
        xy = np.zeros((n, 2), dtype=np.float32)
        pts = np.zeros((n, 3), dtype=np.float32)
        if n:
            self._check(self._lib.velo_get_projection(self._h, C.c_void_p(xy.ctypes.data), C.c_void_p(pts.ctypes.data), n,
                                                      C.c_void_p(off.ctypes.data), off.size, C.byref(nr)))
        return xy, pts, off

    def depth_association(self, keypoints_xy, thresh: float = 0.015):
        """featureDepthAssociation against the last project_lidar: (kp_with_depth [m,3] f32, has_depth [n] i32)."""
        kp = np.ascontiguousarray(np.asarray(keypoints_xy, dtype=np.float32).reshape(-1, 2))
        n = len(kp)
        has = np.full(n, -1, dtype=np.int32)
        out = np.zeros((max(n, 1), 3), dtype=np.float32)
        m = C.c_int32(0)
        self._check(self._lib.velo_depth_association(self._h, C.c_void_p(kp.ctypes.data) if n else None, n, float(thresh),
                                                     C.c_void_p(out.ctypes.data), n, C.c_void_p(has.ctypes.data) if n else None,
                                                     C.byref(m)))
        return out[:m.value].copy(), has

    # -- batched landmark triangulation (velo.h:1027-1130) ---------------------------------------------------------
    def triangulate_points(self, camera_poses, cam_trans, obs, obs_offsets, points_xyz, initial_guess=None):
        """All landmarks of a frame in one call: (points [n,3] f32, results [n] TRI_RESULT_DTYPE).  `points_xyz` supplies the
        initial guesses of the landmarks flagged in `initial_guess`; it is not modified."""
        args = pack_triangulation(camera_poses, cam_trans, obs, obs_offsets, points_xyz, initial_guess)
        poses, ct, ob, off, pts, init = args
        n = len(off) - 1
        res = np.zeros(n, dtype=TRI_RESULT_DTYPE)
        vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None and a.size else None   # noqa: E731
        self._check(self._lib.velo_triangulate_points(self._h, vp(poses), len(poses), vp(ct), len(ct), vp(ob), vp(off), n,
                                                      vp(pts), vp(init), vp(res)))
        return pts, res

    # -- the resident landmark store (main.cpp:614-679, getLandmarksAtFrame velo.h:1132-1160) ---------------------------
    def landmarks_reset(self, cam_trans, log_capacity: int = 0):
        """Empties the store; cam_trans [n_cams, 3] fixes the cameras.  log_capacity: entries before the observation log first
        reallocates (0: the library's default)."""
        ct = np.ascontiguousarray(np.asarray(cam_trans, dtype=np.float32).reshape(-1, 3))
        self._check(self._lib.velo_landmarks_reset(self._h, len(ct), C.c_void_p(ct.ctypes.data), int(log_capacity)))

    def landmarks_set_pose(self, frame: int, pose6):
        x = _dvec(pose6, 6)
        self._check(self._lib.velo_landmarks_set_pose(self._h, int(frame), _ptr(x)))

    def landmarks_observe(self, frame: int, cam: int, ids, keypoints_xy, has_depth, kp_with_depth_xyz=None):
        """keypoints[cam][frame] with their ids, has_depth (-1 or an index into kp_with_depth_xyz [m, 3]) -- main.cpp:622-645"""
        i = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
        k = np.ascontiguousarray(np.asarray(keypoints_xy, dtype=np.float32).reshape(-1, 2))
        h = np.ascontiguousarray(np.asarray(has_depth, dtype=np.int32).reshape(-1))
        d = np.ascontiguousarray(np.asarray(np.zeros((0, 3)) if kp_with_depth_xyz is None else kp_with_depth_xyz, dtype=np.float32).reshape(-1, 3))
        if not len(i) == len(k) == len(h):
            raise ValueError("landmarks_observe: one keypoint and one has_depth entry per id")
        vp = lambda a: C.c_void_p(a.ctypes.data) if a.size else None   # noqa: E731
        self._check(self._lib.velo_landmarks_observe(self._h, int(frame), int(cam), vp(i), vp(k), vp(h), vp(d), len(d), len(i)))

    def landmarks_triangulate(self, frame: int, capacity: Optional[int] = None):
        """main.cpp:654-679 for `frame`: (ids [k] i32 ascending, points [k, 3] f32, results [k] TRI_RESULT_DTYPE).  capacity: the
        raw call with caller-sized outputs, which also returns the count: (ids, points, results, n)."""
        ids, pts, res, n = landmarks_triangulate_batch([self], [frame], capacity=capacity, raw=True)
        if capacity is not None:
            return ids[0], pts[0], res[0], int(n[0])
        return ids[0][:n[0]].copy(), pts[0][:n[0]].copy(), res[0][:n[0]].copy()

    def landmarks_at_frame(self, frame: int, pose_inv, capacity: Optional[int] = None):
        """getLandmarksAtFrame: (ids [k] i32 ascending, xyz [k, 3] f32) of the added landmarks seen in `frame`, in the frame whose
        INVERSE pose (4 x 4) is given.  capacity: caller-sized outputs, returns (ids, xyz, n)."""
        M = _dvec(pose_inv, 16)
        n = C.c_int32(0)
        cap = int(capacity) if capacity is not None else 0
        if capacity is None:                         # the count first: it needs no device work
            self._check(self._lib.velo_landmarks_at_frame(self._h, int(frame), _ptr(M), None, None, 0, C.byref(n)))
            cap = n.value
        ids = np.zeros(max(cap, 1), dtype=np.int32)
        xyz = np.zeros((max(cap, 1), 3), dtype=np.float32)
        self._check(self._lib.velo_landmarks_at_frame(self._h, int(frame), _ptr(M), C.c_void_p(ids.ctypes.data), C.c_void_p(xyz.ctypes.data),
                                                      cap, C.byref(n)))
        if capacity is not None:
            return ids[:cap], xyz[:cap], n.value
        return ids[:n.value].copy(), xyz[:n.value].copy()

    def landmarks_get(self, ids):
        """(xyz [n, 3] f32, added [n] bool, obs_count [n] i32) of the given ids, read from the device"""
        i = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
        n = len(i)
        xyz = np.zeros((max(n, 1), 3), dtype=np.float32)
        added = np.zeros(max(n, 1), dtype=np.uint8)
        cnt = np.zeros(max(n, 1), dtype=np.int32)
        vp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
        self._check(self._lib.velo_landmarks_get(self._h, vp(i) if n else None, n, vp(xyz), vp(added), vp(cnt)))
        return xyz[:n], added[:n].astype(bool), cnt[:n]

    def landmarks_frame_count(self, frame: int):
        """(distinct ids observed in `frame`, how many of them landmarks_triangulate would solve now); host bookkeeping only"""
        a, b = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.velo_landmarks_frame_count(self._h, int(frame), C.byref(a), C.byref(b)))
        return a.value, b.value

    def landmarks_info(self) -> dict:
        a = np.zeros(8, dtype=np.int32)
        self._check(self._lib.velo_landmarks_info(self._h, C.c_void_p(a.ctypes.data)))
        return dict(n_ids=int(a[0]), log_entries=int(a[1]), log_capacity=int(a[2]), log_reallocations=int(a[3]), frame_capacity=int(a[4]),
                    n_cams=int(a[5]), observed=int(a[6]))

    # -- bundle adjustment of a window of frames over the landmark store (main.cpp:673-725) ----------------------------------
    @staticmethod
    def _ba_arguments(frames, weight_3d):
        fr = np.ascontiguousarray(np.asarray(frames, dtype=np.int32).reshape(-1))
        p = VeloBaParams()
        p.weight_3d = float(weight_3d)
        return fr, p

    def landmarks_adjust(self, frames, n_fixed: int = 1, weight_3d: float = 1.0):
        """Bundle-adjusts the window `frames` (ascending; the first n_fixed are constants) over the store's observations:
        (poses [n_frames, 6] f64 -- the fixed frames as they were, the free ones refined --, VeloBaSummary).  The points and the
        store's frame table are updated; summary.trace[:summary.n_trace] holds one record per LM iteration."""
        fr, p = self._ba_arguments(frames, weight_3d)
        poses = np.zeros((max(len(fr), 1), 6), dtype=np.float64)
        s = VeloBaSummary()
        self._check(self._lib.velo_landmarks_adjust(self._h, C.c_void_p(fr.ctypes.data) if len(fr) else None, len(fr), int(n_fixed), C.byref(p),
                                                    C.c_void_p(poses.ctypes.data), C.byref(s)))
        return poses[:len(fr)], s

    def landmarks_adjust_system(self, frames, n_fixed: int = 1, weight_3d: float = 1.0):
        """The problem landmarks_adjust would solve, evaluated at the stored state (nothing changes): (cost, the poses' part of
        J^T r [6 n_free], the poses' diagonal blocks of J^T J [n_free, 6, 6])"""
        fr, p = self._ba_arguments(frames, weight_3d)
        n_free = max(len(fr) - int(n_fixed), 1)
        cost = C.c_double(0.0)
        g = np.zeros(6 * n_free, dtype=np.float64)
        H = np.zeros((n_free, 6, 6), dtype=np.float64)
        self._check(self._lib.velo_landmarks_adjust_system(self._h, C.c_void_p(fr.ctypes.data) if len(fr) else None, len(fr), int(n_fixed), C.byref(p),
                                                           C.byref(cost), C.c_void_p(g.ctypes.data), C.c_void_p(H.ctypes.data)))
        return cost.value, g, H

    # -- the pose graph of a drive and its batch optimisation (main.cpp:190-204, 516-536, 728-745) ------------------------------
    def graph_reset(self, edge_capacity: int = 0):
        """Creates or empties the context's pose graph.  edge_capacity: edges before the device arrays first reallocate (0: the
        library's default)."""
        self._check(self._lib.velo_graph_reset(self._h, int(edge_capacity)))

    def graph_set_pose(self, frame: int, pose6):
        x = _dvec(pose6, 6)
        self._check(self._lib.velo_graph_set_pose(self._h, int(frame), _ptr(x)))

    def graph_set_poses(self, first: int, poses):
        """the nodes first .. first + n - 1 from poses [n, 6]"""
        x = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 6))
        self._check(self._lib.velo_graph_set_poses(self._h, int(first), len(x), C.c_void_p(x.ctypes.data) if len(x) else None))

    def graph_add_edges(self, frm, to, z, info):
        """appends the edges (frm[k], to[k], z[k] (6 doubles: angle-axis, translation of Z with pose_to = pose_from . Z), info[k])"""
        a = np.ascontiguousarray(np.asarray(frm, dtype=np.int32).reshape(-1))
        b = np.ascontiguousarray(np.asarray(to, dtype=np.int32).reshape(-1))
        zz = np.ascontiguousarray(np.asarray(z, dtype=np.float64).reshape(-1, 6))
        w = np.ascontiguousarray(np.asarray(info, dtype=np.float64).reshape(-1))
        if not len(a) == len(b) == len(zz) == len(w):
            raise ValueError("graph_add_edges: one from, to, z and info per edge")
        vp = lambda v: C.c_void_p(v.ctypes.data) if v.size else None   # noqa: E731
        self._check(self._lib.velo_graph_add_edges(self._h, len(a), vp(a), vp(b), vp(zz), vp(w)))

    def graph_add_edges_weighted(self, frm, to, z, info, loss_scale=None):
        """appends edges with a 6 x 6 information W each and, optionally, a robust loss.  info: [n, 6, 6] (symmetric) or [n, 21], W's
        upper triangle row by row; loss_scale [n] or None (all trivial): 0 = trivial, a > 0 = Cauchy(a) on s = r^T W r."""
        a = np.ascontiguousarray(np.asarray(frm, dtype=np.int32).reshape(-1))
        b = np.ascontiguousarray(np.asarray(to, dtype=np.int32).reshape(-1))
        zz = np.ascontiguousarray(np.asarray(z, dtype=np.float64).reshape(-1, 6))
        w = np.asarray(info, dtype=np.float64)
        if w.ndim == 3 and w.shape[1:] == (6, 6):
            if not np.array_equal(w, np.transpose(w, (0, 2, 1))):
                raise ValueError("graph_add_edges_weighted: an information matrix is not symmetric")
            w = w[:, np.triu_indices(6)[0], np.triu_indices(6)[1]]
        elif not (w.ndim == 2 and w.shape[1] == 21):
            raise ValueError("graph_add_edges_weighted: info is [n, 6, 6] or [n, 21]")
        w = np.ascontiguousarray(w)
        ls = None if loss_scale is None else np.ascontiguousarray(np.asarray(loss_scale, dtype=np.float64).reshape(-1))
        if not len(a) == len(b) == len(zz) == len(w) or (ls is not None and len(ls) != len(a)):
            raise ValueError("graph_add_edges_weighted: one from, to, z, info and loss_scale per edge")
        vp = lambda v: C.c_void_p(v.ctypes.data) if v is not None and v.size else None   # noqa: E731
        self._check(self._lib.velo_graph_add_edges_weighted(self._h, len(a), vp(a), vp(b), vp(zz), vp(w), vp(ls)))

    def graph_edge_stats(self, first: int = 0, n: Optional[int] = None):
        """(chi2, weight) of the edges first .. first + n - 1 (None: to the last) at the stored poses, in the order they were added:
        chi2 = r^T W r, weight = rho'(chi2), 1 for a trivial loss.  Nothing changes."""
        if n is None:
            n = self.graph_info()["n_edges"] - int(first)
        chi2 = np.zeros(max(int(n), 1), dtype=np.float64)
        weight = np.zeros(max(int(n), 1), dtype=np.float64)
        self._check(self._lib.velo_graph_edge_stats(self._h, int(first), int(n), C.c_void_p(chi2.ctypes.data), C.c_void_p(weight.ctypes.data)))
        return chi2[:max(int(n), 0)], weight[:max(int(n), 0)]

    @staticmethod
    def _graph_params(cg_tolerance, cg_max_iterations, linear_solver="cg", max_work=None):
        if linear_solver not in GRAPH_SOLVERS and not isinstance(linear_solver, int):
            raise ValueError(f"graph_optimize: linear_solver {linear_solver!r}; one of {sorted(GRAPH_SOLVERS)}")
        solver = GRAPH_SOLVERS.get(linear_solver, linear_solver)
        if cg_tolerance is None and cg_max_iterations is None and solver == GRAPH_SOLVER_CG and max_work is None:
            return None
        p = VeloGraphParams()
        p.cg_tolerance = 1e-10 if cg_tolerance is None else float(cg_tolerance)
        p.cg_max_iterations = 2000 if cg_max_iterations is None else int(cg_max_iterations)
        p.reserved[0] = int(solver)
        p.reserved[1] = 0 if max_work is None else int(max_work)
        return C.byref(p)

    def graph_optimize(self, fixed=(0,), cg_tolerance=None, cg_max_iterations=None, linear_solver="cg", max_work=None) -> "VeloGraphSummary":
        """Refines every node that has a pose and is not in `fixed` (ascending frame numbers) over all edges; the poses are read
        with graph_get_poses.  summary.trace[:summary.n_trace] holds one record per LM iteration.  linear_solver: "cg" (the
        block-Jacobi CG) or "envelope" (the exact envelope Cholesky in reverse Cuthill-McKee order; max_work caps its block products
        per factorisation, None: the library's default; a graph over the cap is refused and nothing changes)."""
        fx = np.ascontiguousarray(np.asarray(fixed, dtype=np.int32).reshape(-1))
        s = VeloGraphSummary()
        self._check(self._lib.velo_graph_optimize(self._h, C.c_void_p(fx.ctypes.data) if len(fx) else None, len(fx),
                                                  self._graph_params(cg_tolerance, cg_max_iterations, linear_solver, max_work), C.byref(s)))
        return s

    def graph_get_poses(self, first: int, n: int) -> np.ndarray:
        out = np.zeros((max(int(n), 1), 6), dtype=np.float64)
        self._check(self._lib.velo_graph_get_poses(self._h, int(first), int(n), C.c_void_p(out.ctypes.data)))
        return out[:int(n)]

    def graph_info(self) -> dict:
        a = np.zeros(8, dtype=np.int32)
        self._check(self._lib.velo_graph_info(self._h, C.c_void_p(a.ctypes.data)))
        return dict(n_nodes=int(a[0]), n_edges=int(a[1]), edge_capacity=int(a[2]), edge_reallocations=int(a[3]), frame_capacity=int(a[4]),
                    optimizations=int(a[5]), envelope_widest_row=int(a[6]), envelope_blocks=int(a[7]))

    def graph_system(self, fixed=(0,), n_free: Optional[int] = None):
        """The problem graph_optimize would solve, evaluated at the stored state (nothing changes): (cost, J^T r [n_free, 6], the
        diagonal blocks of J^T J [n_free, 6, 6]); the free nodes are the nodes with a pose that are not fixed, ascending."""
        fx = np.ascontiguousarray(np.asarray(fixed, dtype=np.int32).reshape(-1))
        if n_free is None:
            n_free = self.graph_info()["n_nodes"] - len(fx)
        n_free = max(int(n_free), 1)
        cost = C.c_double(0.0)
        g = np.zeros((n_free, 6), dtype=np.float64)
        H = np.zeros((n_free, 6, 6), dtype=np.float64)
        self._check(self._lib.velo_graph_system(self._h, C.c_void_p(fx.ctypes.data) if len(fx) else None, len(fx), C.byref(cost),
                                                C.c_void_p(g.ctypes.data), C.c_void_p(H.ctypes.data)))
        return cost.value, g, H

    def graph_covariance(self, pairs_or_frames, fixed=(0,), max_work=None) -> np.ndarray:
        """Covariances of the poses at the stored state (nothing changes): blocks of (J^T J)^-1 of the problem graph_optimize would
        solve, in the coordinates of a node's 6 doubles.  A 1-D list of frames asks for their marginals, an [n, 2] array for
        Cov(a, b) per row (a == b: the marginal; otherwise the cross block, not its transpose); returns [n, 6, 6].  A fixed frame's
        block is zero.  max_work caps the envelope factorisation's block products (None: the library's default).  Refused: what
        graph_optimize refuses, a frame without a pose, and a J^T J that is not positive definite (a free node without edges)."""
        q = np.asarray(pairs_or_frames)
        if q.size and not np.issubdtype(q.dtype, np.integer):
            raise ValueError("graph_covariance: frames are integers")
        if q.ndim == 1:
            q = np.stack([q, q], axis=1) if q.size else np.zeros((0, 2), dtype=np.int32)
        elif q.ndim != 2 or q.shape[1] != 2:
            raise ValueError("graph_covariance: a 1-D list of frames (marginals) or an [n, 2] array of pairs")
        a = np.ascontiguousarray(q[:, 0], dtype=np.int32)
        b = np.ascontiguousarray(q[:, 1], dtype=np.int32)
        fx = np.ascontiguousarray(np.asarray(fixed, dtype=np.int32).reshape(-1))
        out = np.zeros((max(len(a), 1), 6, 6), dtype=np.float64)
        params = None
        if max_work is not None:
            params = self._graph_params(None, None, "cg", max_work)
        vp = lambda v: C.c_void_p(v.ctypes.data) if len(v) else None  # noqa: E731
        self._check(self._lib.velo_graph_covariance(self._h, vp(fx), len(fx), params, len(a), vp(a), vp(b), C.c_void_p(out.ctypes.data)))
        return out[:len(a)]

    def graph_joint_covariance(self, a: int, b: int, fixed=(0,)) -> np.ndarray:
        """The 12 x 12 joint covariance of frames a and b, from the three blocks of one graph_covariance call; symmetric by construction:
        its (b, a) block is the transpose of the returned (a, b) block."""
        blk = self.graph_covariance([[a, a], [a, b], [b, b]], fixed)
        J = np.empty((12, 12), dtype=np.float64)
        J[:6, :6], J[:6, 6:], J[6:, :6], J[6:, 6:] = blk[0], blk[1], blk[1].T, blk[2]
        return J

    def graph_edge_gate(self, frm, to, z=None, info=None, fixed=(0,), max_work=None):
        """velo_graph_edge_gate: proposed edges (frm[k], to[k], z[k], info[k]) tested against the graph BEFORE they enter it, at the
        stored state (nothing changes; optimise first: the covariance belongs to the optimum).  Returns (rel [n, 6], r [n, 6],
        cov [n, 6, 6], chi2 [n]): the stored relative pose, the unweighted edge residual, S = Sigma_rel + W^-1 and r^T S^-1 r (-1 where
        S is not positive definite), to be compared with a chi-square quantile of 6 degrees of freedom.  z None: every pair's own
        relative pose (r is then zero to rounding); info: [n, 6, 6] or [n, 21] as in graph_add_edges_weighted, None: S = Sigma_rel."""
        a = np.ascontiguousarray(np.asarray(frm, dtype=np.int32).reshape(-1))
        b = np.ascontiguousarray(np.asarray(to, dtype=np.int32).reshape(-1))
        zz = None if z is None else np.ascontiguousarray(np.asarray(z, dtype=np.float64).reshape(-1, 6))
        w = None
        if info is not None:
            w = np.asarray(info, dtype=np.float64)
            if w.ndim == 3 and w.shape[1:] == (6, 6):
                if not np.array_equal(w, np.transpose(w, (0, 2, 1))):
                    raise ValueError("graph_edge_gate: an information matrix is not symmetric")
                w = w[:, np.triu_indices(6)[0], np.triu_indices(6)[1]]
            elif not (w.ndim == 2 and w.shape[1] == 21):
                raise ValueError("graph_edge_gate: info is [n, 6, 6] or [n, 21]")
            w = np.ascontiguousarray(w)
        if len(a) != len(b) or (zz is not None and len(zz) != len(a)) or (w is not None and len(w) != len(a)):
            raise ValueError("graph_edge_gate: one from, to, z and info per pair")
        fx = np.ascontiguousarray(np.asarray(fixed, dtype=np.int32).reshape(-1))
        n = len(a)
        rel, r = np.zeros((max(n, 1), 6)), np.zeros((max(n, 1), 6))
        cov, chi2 = np.zeros((max(n, 1), 6, 6)), np.zeros(max(n, 1))
        params = None if max_work is None else self._graph_params(None, None, "cg", max_work)
        vp = lambda v: C.c_void_p(v.ctypes.data) if v is not None and v.size else None   # noqa: E731
        self._check(self._lib.velo_graph_edge_gate(self._h, vp(fx), len(fx), params, n, vp(a), vp(b), vp(zz), vp(w), vp(rel), vp(r), vp(cov), vp(chi2)))
        return rel[:n], r[:n], cov[:n], chi2[:n]

    def graph_relative_covariance(self, pairs, fixed=(0,)):
        """(rel [n, 6], cov [n, 6, 6]) for an [n, 2] array of frames (a, b): the stored relative pose pose_vec(T_a^-1 T_b) and its
        covariance in the tangent at that pose -- graph_edge_gate without a measurement and without an information.  Unlike the
        marginals of graph_covariance it does not depend on which frame is fixed."""
        q = np.asarray(pairs)
        if q.size and not np.issubdtype(q.dtype, np.integer):
            raise ValueError("graph_relative_covariance: frames are integers")
        if q.size == 0:
            q = np.zeros((0, 2), dtype=np.int32)
        if q.ndim != 2 or q.shape[1] != 2:
            raise ValueError("graph_relative_covariance: an [n, 2] array of pairs")
        rel, _, cov, _ = self.graph_edge_gate(q[:, 0], q[:, 1], None, None, fixed)
        return rel, cov

    def graph_loop_candidates(self, query: int, min_gap: int, radius: float, k_sigma: float = 0.0, fixed=(0,), capacity: Optional[int] = None,
                              max_work=None):
        """velo_graph_loop_candidates: (frames, dist, sigma) of the frames i with |i - query| >= min_gap whose stored distance to the
        query is at most radius + k_sigma . sigma_i, ascending; sigma_i is the standard deviation of the relative position from the
        graph (0 with k_sigma == 0, which runs no factorisation).  capacity: the room of the first call (None: 64); a call that finds
        more is repeated with that room -- a second whole call, factorisation included, so give the room at once where more can be
        expected.  max_work caps the envelope factorisation's block products (None: the library's default)."""
        fx = np.ascontiguousarray(np.asarray(fixed, dtype=np.int32).reshape(-1))
        cap = 64 if capacity is None else int(capacity)
        params = None if max_work is None else self._graph_params(None, None, "cg", max_work)
        vp = lambda v: C.c_void_p(v.ctypes.data) if v.size else None   # noqa: E731
        while True:
            frames = np.zeros(max(cap, 1), dtype=np.int32)
            dist, sigma = np.zeros(max(cap, 1)), np.zeros(max(cap, 1))
            found = C.c_int32(0)
            self._check(self._lib.velo_graph_loop_candidates(self._h, vp(fx), len(fx), params, int(query), int(min_gap), float(radius), float(k_sigma), cap,
                                                             vp(frames), vp(dist), vp(sigma), C.byref(found)))
            if found.value <= cap:
                return frames[:found.value], dist[:found.value], sigma[:found.value]
            cap = found.value

    def graph_retain(self, fixed=(0,), max_work=None, perm=None):
        """velo_graph_retain: keeps the factorisation graph_covariance, graph_edge_gate and graph_loop_candidates (k_sigma > 0) build for
        this `fixed` set, so that they stop building it per call; appended frames and edges extend it from the first row they touch.
        perm: the order of the free nodes' indices to factor in (with api.graph_order's the answers are an un-retained call's to the
        bit); None: frame order unless that costs more than twice the fresh order.  Retain again after graph_optimize."""
        fx = np.ascontiguousarray(np.asarray(fixed, dtype=np.int32).reshape(-1))
        pm = None if perm is None else np.ascontiguousarray(np.asarray(perm, dtype=np.int32).reshape(-1))
        params = None if max_work is None else self._graph_params(None, None, "cg", max_work)
        one = np.zeros(1, dtype=np.int32)                              # (an empty order is still an order: not NULL)
        self._check(self._lib.velo_graph_retain(self._h, C.c_void_p(fx.ctypes.data) if len(fx) else None, len(fx), params,
                                                None if pm is None else C.c_void_p((pm if len(pm) else one).ctypes.data), 0 if pm is None else len(pm)))

    def graph_release(self):
        """velo_graph_release: forgets the retained factorisation (none is fine)"""
        self._check(self._lib.velo_graph_release(self._h))

    def graph_retained(self) -> dict:
        """velo_graph_retained: the retained factorisation's state ("none", "current", "behind" as state 0, 1, 2), its size, the counters
        that show what work was skipped, and its order `perm` (free indices by position)."""
        info = np.zeros(16, dtype=np.int64)
        self._check(self._lib.velo_graph_retained(self._h, C.c_void_p(info.ctypes.data), None, 0))
        perm = np.zeros(max(int(info[1]), 1), dtype=np.int32)
        self._check(self._lib.velo_graph_retained(self._h, C.c_void_p(info.ctypes.data), C.c_void_p(perm.ctypes.data), int(info[1])))
        keys = ("state", "n_free", "widest_row", "blocks", "work", "builds", "extensions", "rebuilds", "selected_inverses", "columns", "served",
                "first_dirty_row", "rows_refactored")
        out = {k: int(info[i]) for i, k in enumerate(keys)}
        out["perm"] = perm[:int(info[1])]
        return out

    # -- resident keypoint frames and the visual matches assembled from them (velo.h:562-590, velo.h:627-654) ---------------
    def frames_reset(self, cam_trans, arena_capacity: int = 0):
        """Empties the frame store; cam_trans [n_cams, 3] fixes the cameras.  arena_capacity: bytes before the arena first
        reallocates (0: the library's default)."""
        ct = np.ascontiguousarray(np.asarray(cam_trans, dtype=np.float32).reshape(-1, 3))
        self._check(self._lib.velo_frames_reset(self._h, len(ct), C.c_void_p(ct.ctypes.data), int(arena_capacity)))
        self._fr_cams = len(ct)

    def frames_put(self, frame: int, cam: int, ids, keypoints_xy, has_depth, kp_with_depth_xyz=None):
        """keypoints[cam][frame] with their ids, has_depth and the depth cloud (the arguments of landmarks_observe); a second put of
        the same (frame, cam) replaces the entry"""
        i = np.ascontiguousarray(np.asarray(ids, dtype=np.int32).reshape(-1))
        k = np.ascontiguousarray(np.asarray(keypoints_xy, dtype=np.float32).reshape(-1, 2))
        h = np.ascontiguousarray(np.asarray(has_depth, dtype=np.int32).reshape(-1))
        d = np.ascontiguousarray(np.asarray(np.zeros((0, 3)) if kp_with_depth_xyz is None else kp_with_depth_xyz, dtype=np.float32).reshape(-1, 3))
        if not len(i) == len(k) == len(h):
            raise ValueError("frames_put: one keypoint and one has_depth entry per id")
        vp = lambda a: C.c_void_p(a.ctypes.data) if a.size else None   # noqa: E731
        self._check(self._lib.velo_frames_put(self._h, int(frame), int(cam), vp(i), vp(k), vp(h), vp(d), len(d), len(i)))

    def frames_drop(self, frame: int):
        self._check(self._lib.velo_frames_drop(self._h, int(frame)))

    def frames_info(self) -> dict:
        a = np.zeros(8, dtype=np.int32)
        self._check(self._lib.velo_frames_info(self._h, C.c_void_p(a.ctypes.data)))
        return dict(frames=int(a[0]), entries=int(a[1]), arena_bytes=int(a[2]), arena_reallocations=int(a[3]), arena_used=int(a[4]),
                    n_cams=int(a[5]), slot_ids=int(a[6]), free_blocks=int(a[7]))

    def frames_count(self, frame: int):
        """(keypoints per camera of `frame` as put, -1 where never put; their sum): host bookkeeping only"""
        a = np.full(8, -1, dtype=np.int32)
        n = C.c_int32(0)
        self._check(self._lib.velo_frames_count(self._h, int(frame), C.c_void_p(a.ctypes.data), C.byref(n)))
        if getattr(self, "_fr_cams", None) is None:
            self._fr_cams = self.frames_info()["n_cams"]
        return a[:self._fr_cams].copy(), n.value

    def build_matches(self, frame1: int, frame2: int, pose2_inv=None, capacity: Optional[int] = None):
        """The visual set of frameToFrame(frame1, frame2) assembled on the device from the frame store (and the landmark store when
        pose2_inv, the 4 x 4 INVERSE pose of frame2, is given): (n_per_cam [n_cams] i32, pairs [n, 2] i32 (point1, point2)), both as
        the call wrote them.  capacity: caller-sized pairs, returns (n_per_cam, pairs [capacity, 2], n)."""
        per_cam, pairs, n, n_cams = build_matches_batch([self], [frame1], [frame2], None if pose2_inv is None else [pose2_inv],
                                                        capacity=capacity, raw=True, _with_cams=True)
        if capacity is not None:
            return per_cam[0, :n_cams[0]].copy(), pairs[0], int(n[0])
        return per_cam[0, :n_cams[0]].copy(), pairs[0, :n[0]].copy()

    def frames_put_descriptors(self, frame: int, cam: int, rows):
        """The FREAK rows (uint8 (n, 64), one per keypoint) of an entry frames_put has made; a second call replaces them"""
        r = np.ascontiguousarray(np.asarray(rows, dtype=np.uint8))
        if r.size == 0:
            r = r.reshape(0, 64)
        if r.ndim != 2 or r.shape[1] != 64:
            raise ValueError(f"descriptors must be uint8 (n, 64), got shape {r.shape}")
        self._check(self._lib.velo_frames_put_descriptors(self._h, int(frame), int(cam), C.c_void_p(r.ctypes.data) if len(r) else None, len(r)))

    def frames_desc_info(self) -> dict:
        a = np.zeros(4, dtype=np.int32)
        self._check(self._lib.velo_frames_desc_info(self._h, C.c_void_p(a.ctypes.data)))
        return dict(entries=int(a[0]), arena_bytes=int(a[1]), arena_reallocations=int(a[2]), free_blocks=int(a[3]))

    def build_matches_desc(self, frame1: int, frame2: int, pose2_inv=None, match_thresh: float = 29.0, capacity: Optional[int] = None):
        """build_matches with the frames joined by their resident descriptor rows (matchFeatures, the loop-closure edge) instead of
        their ids: query = frame1, train = frame2, pairs (point1, point2) = (queryIdx, trainIdx).  Returns what build_matches returns."""
        per_cam, pairs, n, n_cams = build_matches_desc_batch([self], [frame1], [frame2], None if pose2_inv is None else [pose2_inv],
                                                             match_thresh, capacity=capacity, raw=True, _with_cams=True)
        if capacity is not None:
            return per_cam[0, :n_cams[0]].copy(), pairs[0], int(n[0])
        return per_cam[0, :n_cams[0]].copy(), pairs[0, :n[0]].copy()

    def match_frames(self, frame1: int, frames2, match_thresh: float = 29.0):
        """frame1's resident rows against those of every candidate frame of frames2, camera by camera, in one launch set:
        (n_kept [n_cand, n_cams] i32, min_dist [n_cand, n_cams] i32, -1 where a side is empty).  The visual set is left alone."""
        f2 = np.ascontiguousarray(np.asarray(frames2, dtype=np.int32).reshape(-1))
        if getattr(self, "_fr_cams", None) is None:
            self._fr_cams = self.frames_info()["n_cams"]
        kept = np.zeros((max(len(f2), 1), self._fr_cams), dtype=np.int32)
        md = np.full((max(len(f2), 1), self._fr_cams), -1, dtype=np.int32)
        vp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
        self._check(self._lib.velo_match_frames(self._h, int(frame1), vp(f2) if len(f2) else None, len(f2), float(match_thresh), vp(kept), vp(md)))
        return kept[:len(f2)], md[:len(f2)]

    # -- pruning a resident frame (removeSlightlyLessTerribleFeatures, velo.h:272-327) ---------------------------------------
    def frames_get(self, frame: int, cam: int):
        """One entry as the store holds it: (ids [n] i32, keypoints [n, 2] f32, has_depth [n] i32, kp_with_depth [m, 3] f32,
        rows uint8 [n, 64] or None when the entry holds no descriptor rows)"""
        n, m, hr = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._check(self._lib.velo_frames_get(self._h, int(frame), int(cam), None, None, None, None, None, 0, 0, C.byref(n), C.byref(m), C.byref(hr)))
        ids, has = np.zeros(n.value, np.int32), np.zeros(n.value, np.int32)
        xy, cloud = np.zeros((n.value, 2), np.float32), np.zeros((m.value, 3), np.float32)
        rows = np.zeros((n.value, 64), np.uint8) if hr.value else None
        vp = lambda a: C.c_void_p(a.ctypes.data) if a is not None and a.size else None   # noqa: E731
        self._check(self._lib.velo_frames_get(self._h, int(frame), int(cam), vp(ids), vp(xy), vp(has), vp(cloud), vp(rows), n.value, m.value,
                                              C.byref(n), C.byref(m), C.byref(hr)))
        return ids, xy, has, cloud, rows

    def frames_keep(self, frame: int, cam: int, keep_idx):
        """Cuts the entry (frame, cam) down to the SET of indices in keep_idx (any order, duplicates allowed) on the device, as
        velo.h:302-325 does; returns (kept old indices, ascending, i32; the entry's new n_with_depth)"""
        k = np.ascontiguousarray(np.asarray(keep_idx, dtype=np.int32).reshape(-1))
        cap = max(int(self.frames_count(frame)[0][cam]), 0) if 0 <= cam < self.frames_info()["n_cams"] else 0
        kept = np.zeros(max(cap, 1), dtype=np.int32)
        n, m = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.velo_frames_keep(self._h, int(frame), int(cam), C.c_void_p(k.ctypes.data) if len(k) else None, len(k),
                                               C.c_void_p(kept.ctypes.data), cap, C.byref(n), C.byref(m)))
        return kept[:n.value].copy(), m.value

    def frames_prune(self, frame: int):
        """removeSlightlyLessTerribleFeatures on the device for every camera of `frame`, the keep set read from the visual set
        build_matches[_desc] made with `frame` as frame1 and the flags of the registration since: per camera the kept old indices
        (ascending, i32), and n_with_depth [n_cams] i32"""
        kept, n_wd = frames_prune_batch([self], [frame])[0]
        return kept, n_wd

    # -- a frame put with its keypoint depth computed on the device (velo.h:329-497 in front of the stores) ------------------
    def frames_put_frame(self, frame: int, cams, thresh: float = 0.015, of_target: bool = False, observe: bool = False) -> np.ndarray:
        """project_lidar + depth_association + frames_put (+ frames_put_descriptors where a FrameCam has rows, + landmarks_observe
        with observe=True) for every camera of the frame store in one call, has_depth and the depth cloud never leaving the device.
        cams: one FrameCam per camera of the store.  Returns n_with_depth [n_cams] i32."""
        return frames_put_frame_batch([self], [frame], [cams], thresh, [of_target], observe)[0]

    def get_visual(self, capacity: Optional[int] = None) -> np.ndarray:
        """The context's device-side visual set (velo_match records), whoever wrote it"""
        n = C.c_int32(0)
        self._check(self._lib.velo_get_visual(self._h, None, 0, C.byref(n)))
        cap = n.value if capacity is None else int(capacity)
        out = np.zeros(max(cap, 1), dtype=MATCH_DTYPE)
        self._check(self._lib.velo_get_visual(self._h, C.c_void_p(out.ctypes.data), cap, C.byref(n)))
        return out[:min(cap, n.value)]

    # -- descriptor matching: matchFeatures (velo.h:499-560) ----------------------------------------------------
    def match_descriptors(self, query, train, match_thresh: float = 29.0):
        """BFMatcher(NORM_HAMMING).match + the velo.h:536-549 filter for one (query, train) pair of uint8 (n, 64) arrays:
        (train_idx [nq] i32, distance [nq] i32, min_dist int, pairs [k, 2] i32 (queryIdx, trainIdx))."""
        idx, dist, md, pairs = self.match_descriptor_jobs([(query, train)], match_thresh)
        return idx[0], dist[0], int(md[0]), pairs[0]

    def match_descriptor_jobs(self, jobs, match_thresh: float = 29.0):
        """Every (query, train) pair of `jobs` in ONE call (one upload, one launch set, one copy back; a set passed as the same array
        object to several jobs travels once): per job lists (train_idx [nq], distance [nq]), min_dist [n_jobs] i32 (-1: no match) and
        a list of the kept (queryIdx, trainIdx) pairs [k, 2]."""
        sets = {}                                             # id(array) -> contiguous uint8 (n, 64): the C side dedupes by pointer
        held = []

        def rows(a):
            key = id(a)
            if key not in sets:
                arr = np.ascontiguousarray(np.asarray(a, dtype=np.uint8))
                if arr.size == 0:
                    arr = arr.reshape(0, 64)
                if arr.ndim != 2 or arr.shape[1] != 64:
                    raise ValueError(f"descriptors must be uint8 (n, 64), got shape {arr.shape}")
                sets[key] = arr
                held.append(a)                                # ids stay unique while the call runs
            return sets[key]

        n_jobs = len(jobs)
        arr = (VeloDescJob * max(n_jobs, 1))()
        nqs = []
        for j, (q, t) in enumerate(jobs):
            qa, ta = rows(q), rows(t)
            arr[j].query = qa.ctypes.data if len(qa) else None
            arr[j].n_query = len(qa)
            arr[j].train = ta.ctypes.data if len(ta) else None
            arr[j].n_train = len(ta)
            nqs.append(len(qa))
        nq = int(sum(nqs))
        idx = np.full(max(nq, 1), -1, dtype=np.int32)
        dist = np.full(max(nq, 1), -1, dtype=np.int32)
        pairs = np.zeros((max(nq, 1), 2), dtype=np.int32)
        md = np.full(max(n_jobs, 1), -1, dtype=np.int32)
        nk = np.zeros(max(n_jobs, 1), dtype=np.int32)
        vp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
        self._check(self._lib.velo_match_descriptors(self._h, C.cast(arr, C.c_void_p), n_jobs, float(match_thresh), vp(idx), vp(dist),
                                                     vp(md), vp(nk), vp(pairs)))
        q_off = np.concatenate([[0], np.cumsum(nqs)]).astype(np.int64)
        k_off = np.concatenate([[0], np.cumsum(nk[:n_jobs])]).astype(np.int64)
        idx_l = [idx[q_off[j]:q_off[j + 1]].copy() for j in range(n_jobs)]
        dist_l = [dist[q_off[j]:q_off[j + 1]].copy() for j in range(n_jobs)]
        pairs_l = [pairs[k_off[j]:k_off[j + 1]].copy() for j in range(n_jobs)]
        return idx_l, dist_l, md[:n_jobs].copy(), pairs_l

    # -- feature tracking: trackFeatures (velo.h:28-116) -----------------------------------------------------------------
    def set_images(self, imgs):
        """The frame's grayscale images (one 2-D uint8 array per camera, all the same shape) become the current ones; the current
        ones become the previous ones.  Pyramids and derivatives are built on the device."""
        arrs = [np.ascontiguousarray(np.asarray(im, dtype=np.uint8)) for im in imgs]
        if not arrs or any(a.ndim != 2 or a.shape != arrs[0].shape for a in arrs):
            raise ValueError("set_images: one or more 2-D uint8 images of one shape")
        h, w = arrs[0].shape
        ptrs = (C.c_void_p * len(arrs))(*[a.ctypes.data for a in arrs])
        self._check(self._lib.velo_set_images(self._h, C.cast(ptrs, C.c_void_p), len(arrs), w, h, w))

    def get_image_level(self, cam: int, level: int = 0, kind: str = "img", previous: bool = False):
        """One stored level, padded: uint8 (image) or int16 (dx / dy) of shape (h + 2 pad, w + 2 pad); returns (array, pad)."""
        dims = np.zeros(4, dtype=np.int32)
        k = IMAGE_KINDS[kind]
        self._check(self._lib.velo_get_image_level(self._h, int(cam), int(bool(previous)), int(level), k, None, 0,
                                                   C.c_void_p(dims.ctypes.data)))
        w, h, pad = int(dims[0]), int(dims[1]), int(dims[2])
        out = np.zeros((h + 2 * pad, w + 2 * pad), dtype=np.uint8 if k == 0 else np.int16)
        self._check(self._lib.velo_get_image_level(self._h, int(cam), int(bool(previous)), int(level), k, C.c_void_p(out.ctypes.data),
                                                   out.nbytes, C.c_void_p(dims.ctypes.data)))
        return out, pad

    def image_levels(self, previous: bool = False) -> int:
        dims = np.zeros(4, dtype=np.int32)
        self._check(self._lib.velo_get_image_level(self._h, 0, int(bool(previous)), 0, 0, None, 0, C.c_void_p(dims.ctypes.data)))
        return int(dims[3])

    def track_features(self, jobs, **params):
        """Every (prev_cam, cam, prev_xy [n, 2] pixels) job in ONE call: per job lists of next_xy [n, 2] f32, status [n] bool and
        kept [n] bool (the filters of velo.h:72-84).  params: lk_params keywords."""
        p = lk_params(**params)
        pts = [np.ascontiguousarray(np.asarray(xy, dtype=np.float32).reshape(-1, 2)) for _, _, xy in jobs]
        arr = (VeloTrackJob * max(len(jobs), 1))()
        for j, ((pc, cc, _), a) in enumerate(zip(jobs, pts)):
            arr[j].prev_cam, arr[j].cam = int(pc), int(cc)
            arr[j].prev_xy = a.ctypes.data if len(a) else None
            arr[j].n = len(a)
        n = int(sum(len(a) for a in pts))
        nxt = np.zeros((max(n, 1), 2), dtype=np.float32)
        st = np.zeros(max(n, 1), dtype=np.uint8)
        kp = np.zeros(max(n, 1), dtype=np.uint8)
        vp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
        self._check(self._lib.velo_track_features(self._h, C.cast(arr, C.c_void_p), len(jobs), C.byref(p), vp(nxt), vp(st), vp(kp)))
        off = np.concatenate([[0], np.cumsum([len(a) for a in pts])]).astype(np.int64)
        return ([nxt[off[j]:off[j + 1]].copy() for j in range(len(jobs))], [st[off[j]:off[j + 1]].astype(bool) for j in range(len(jobs))],
                [kp[off[j]:off[j + 1]].astype(bool) for j in range(len(jobs))])

    # -- corner detection: detectFeatures (velo.h:118-177) ---------------------------------------------------------------
    def current_image_size(self):
        """(width, height) of the current images"""
        dims = np.zeros(4, dtype=np.int32)
        self._check(self._lib.velo_get_image_level(self._h, 0, 0, 0, 0, None, 0, C.c_void_p(dims.ctypes.data)))
        return int(dims[0]), int(dims[1])

    def corner_response(self, cam: int) -> np.ndarray:
        """The minimum-eigenvalue map (cornerMinEigenVal, 3 x 3 / 3 x 3) of the current image of cam: float32 [height, width]"""
        w, h = self.current_image_size()
        out = np.zeros((h, w), dtype=np.float32)
        self._check(self._lib.velo_get_corner_response(self._h, int(cam), C.c_void_p(out.ctypes.data), out.nbytes))
        return out

    def detect_features_raw(self, jobs, capacity: int, xy=None, response=None, fresh=None, **params):
        """velo_detect_features as it is: jobs = [(cam, existing_xy [n, 2] or None)]; returns the caller-sized arrays
        (xy [n_jobs, capacity, 2], response, fresh, counts [n_jobs, 3]); arrays handed in are written in place"""
        p = gftt_params(**params)
        n_jobs = len(jobs)
        pts = [np.ascontiguousarray(np.asarray(np.zeros((0, 2)) if e is None else e, dtype=np.float32).reshape(-1, 2)) for _, e in jobs]
        arr = (VeloDetectJob * max(n_jobs, 1))()
        for j, ((cam, _), a) in enumerate(zip(jobs, pts)):
            arr[j].cam, arr[j].n_existing = int(cam), len(a)
            arr[j].existing_xy = a.ctypes.data if len(a) else None
        cap = int(capacity)
        xy = np.zeros((max(n_jobs, 1), max(cap, 1), 2), dtype=np.float32) if xy is None else xy
        response = np.zeros((max(n_jobs, 1), max(cap, 1)), dtype=np.float32) if response is None else response
        fresh = np.zeros((max(n_jobs, 1), max(cap, 1)), dtype=np.uint8) if fresh is None else fresh
        counts = np.zeros((max(n_jobs, 1), 3), dtype=np.int32)
        vp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
        self._check(self._lib.velo_detect_features(self._h, C.cast(arr, C.c_void_p), n_jobs, C.byref(p), cap, vp(xy), vp(response),
                                                   vp(fresh), vp(counts)))
        return xy, response, fresh, counts[:n_jobs]

    def detect_features(self, jobs, return_counts: bool = False, **params):
        """Every (cam, existing_xy [n, 2] pixels or None) job in ONE call on the current images: per job (xy [k, 2] f32, response [k]
        f32, fresh [k] bool) in selection order.  params: gftt_params keywords (max_corners, quality_level, min_distance)."""
        p = gftt_params(**params)
        w, h = self.current_image_size()
        cap = p.max_corners if p.max_corners > 0 else 4096
        while True:
            xy, resp, fr, counts = self.detect_features_raw(jobs, cap, **params)
            need = int(counts[:, 0].max()) if len(jobs) else 0
            if need <= cap:
                break
            cap = min(need, w * h)                  # no cap on the corners and more of them than assumed: once more, sized right
        res = [(xy[j, :counts[j, 0]].copy(), resp[j, :counts[j, 0]].copy(), fr[j, :counts[j, 0]].astype(bool)) for j in range(len(jobs))]
        return (res, counts.copy()) if return_counts else res

    # -- multi-GPU -------------------------------------------------------------------------------------------
    def set_query_shard(self, rank: int, world: int):
        self._check(self._lib.velo_set_query_shard(self._h, int(rank), int(world)))

    def comm_init(self, unique_id: bytes, rank: int, world: int):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        self._check(self._lib.velo_comm_init(self._h, buf, int(rank), int(world)))

    def comm_destroy(self):
        self._check(self._lib.velo_comm_destroy(self._h))

    def comm_peer_export(self) -> bytes:
        """IPC handle (64 bytes) of this context's all-reduce slab; gather the handles of all ranks, then comm_peer_attach."""
        buf = C.create_string_buffer(64)
        self._check(self._lib.velo_comm_peer_export(self._h, buf))
        return buf.raw

    def comm_peer_attach(self, handles, rank: int, world: int):
        blob = b"".join(bytes(h) for h in handles)
        if len(blob) != 64 * world:
            raise ValueError("one 64-byte handle per rank, in rank order")
        self._check(self._lib.velo_comm_peer_attach(self._h, C.create_string_buffer(blob, len(blob)), int(rank), int(world)))

    def comm_peer_export_records(self, max_queries: int) -> bytes:
        buf = C.create_string_buffer(64)
        self._check(self._lib.velo_comm_peer_export_records(self._h, int(max_queries), buf))
        return buf.raw

    def comm_peer_attach_records(self, handles, max_queries: int):
        blob = b"".join(bytes(h) for h in handles)
        self._check(self._lib.velo_comm_peer_attach_records(self._h, C.create_string_buffer(blob, len(blob)), int(max_queries)))

    def set_residual_stats(self, enable: bool = True):
        """residualStats after every f2f iteration into the summary (velo.h:909)."""
        self._check(self._lib.velo_set_residual_stats(self._h, 1 if enable else 0))

    def residual_stats(self, x):
        """residualStats (velo.h:921-1025) of the current blocks at x."""
        xx = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(6))
        out = VeloResidualStats()
        self._check(self._lib.velo_residual_stats_at(self._h, _ptr(xx), C.byref(out)))
        return out

    def chain_stats(self):
        """(calls, misses) of the one-chain-per-call mode (velo_chain_stats): misses were repeated host-driven, same results."""
        a, b = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.velo_chain_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def comm_info(self):
        """(kind, rank, world): kind 0 = none, 1 = RCCL (world read back from the communicator), 2 = peer slabs."""
        k, r, w = C.c_int32(0), C.c_int32(0), C.c_int32(0)
        self._check(self._lib.velo_comm_info(self._h, C.byref(k), C.byref(r), C.byref(w)))
        return k.value, r.value, w.value


class ScanCache:
    """Device-resident scan cache (velo_cache_*): the reference's ScansLRU (lru.h:31-61, 50 scans) with the scans and their
    search index kept in HBM.  store() copies the scan a context holds; load() hands it to any context as target or source."""

    def __init__(self, device: int = 0, capacity: int = 50, lib: Optional[C.CDLL] = None):
        self._lib = lib if lib is not None else load_library()
        self._h = C.c_void_p()
        status = self._lib.velo_cache_create(C.byref(self._h), int(device), int(capacity))
        if status != 0:
            msg = self._lib.velo_last_error()
            raise VeloError(f"velo status {status}: {msg.decode() if msg else ''}")

    def _check(self, status: int):
        if status != 0:
            msg = self._lib.velo_last_error()
            raise VeloError(f"velo status {status}: {msg.decode() if msg else ''}")

    def close(self):
        if self._h:
            self._lib.velo_cache_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def store(self, frame: int, ctx: "Context", of_target: bool):
        self._check(self._lib.velo_cache_store(self._h, int(frame), ctx.handle, int(bool(of_target))))

    def load(self, frame: int, ctx: "Context", as_target: bool):
        self._check(self._lib.velo_cache_load(self._h, int(frame), ctx.handle, int(bool(as_target))))

    def __contains__(self, frame: int) -> bool:
        return bool(self._lib.velo_cache_contains(self._h, int(frame)))

    def frames(self):
        """cached frame numbers, most recently used first"""
        n = self._lib.velo_cache_frames(self._h, None, 0)
        out = (C.c_int32 * max(n, 1))()
        n = self._lib.velo_cache_frames(self._h, out, n)
        return [int(out[i]) for i in range(n)]


MAP_INFO_FIELDS = ("scans", "points", "rings", "max_scans", "max_points", "evictions", "arena_points", "arena_growths")


class ScanMap:
    """Device-resident sliding-window scan map (velo_map_*): every scan as it was registered, in its own sensor frame, with a pose;
    load() writes the window into a context as its target in the frame the caller names (ref_inv: the INVERSE of the reference pose)."""

    def __init__(self, device: int = 0, max_scans: int = 17, max_points: int = 1 << 22, lib: Optional[C.CDLL] = None):
        self._lib = lib if lib is not None else load_library()
        self._h = C.c_void_p()
        status = self._lib.velo_map_create(C.byref(self._h), int(device), int(max_scans), int(max_points))
        if status != 0:
            msg = self._lib.velo_last_error()
            raise VeloError(f"velo status {status}: {msg.decode() if msg else ''}")

    def _check(self, status: int):
        if status != 0:
            msg = self._lib.velo_last_error()
            raise VeloError(f"velo status {status}: {msg.decode() if msg else ''}")

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            self._lib.velo_map_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def insert(self, ctx: "Context", of_target: bool, frame: int, pose) -> int:
        """the scan `ctx` holds enters under `frame` with its pose (4 x 4); returns how many of the oldest scans went for it"""
        p = _dvec(pose, 16)
        gone = C.c_int32(0)
        self._check(self._lib.velo_map_insert(self._h, ctx.handle, int(bool(of_target)), int(frame), _ptr(p), C.byref(gone)))
        return gone.value

    def set_pose(self, frame: int, pose):
        p = _dvec(pose, 16)
        self._check(self._lib.velo_map_set_pose(self._h, int(frame), _ptr(p)))

    def drop(self, frame: int):
        self._check(self._lib.velo_map_drop(self._h, int(frame)))

    def clear(self):
        self._check(self._lib.velo_map_clear(self._h))

    def frames(self):
        """frame numbers, oldest first"""
        n = self._lib.velo_map_frames(self._h, None, 0)
        out = (C.c_int32 * max(n, 1))()
        n = self._lib.velo_map_frames(self._h, out, n)
        return [int(out[i]) for i in range(n)]

    def info(self) -> dict:
        v = (C.c_int64 * 8)()
        self._check(self._lib.velo_map_info(self._h, v))
        return dict(zip(MAP_INFO_FIELDS, (int(x) for x in v)))

    def get_scan(self, frame: int):
        """(xyz [n, 3] float32, ring offsets int32, pose [4, 4]) of one stored scan"""
        n, r = C.c_int32(0), C.c_int32(0)
        self._check(self._lib.velo_map_get_scan(self._h, int(frame), None, 0, C.byref(n), None, 0, C.byref(r), None))
        xyz = np.zeros((max(n.value, 1), 3), dtype=np.float32)
        off = np.zeros(r.value + 1, dtype=np.int32)
        pose = np.zeros(16)
        self._check(self._lib.velo_map_get_scan(self._h, int(frame), xyz.ctypes.data_as(C.c_void_p), n.value, C.byref(n),
                                                off.ctypes.data_as(C.c_void_p), r.value + 1, C.byref(r), _ptr(pose)))
        return xyz[:n.value], off, pose.reshape(4, 4)

    def load(self, ctx: "Context", ref_inv):
        p = _dvec(ref_inv, 16)
        self._check(self._lib.velo_map_load(self._h, ctx.handle, _ptr(p)))


def map_load_batch(maps, ctxs, ref_invs):
    """ScanMap.load for every (maps[i], ctxs[i], ref_invs[i]) in ONE call: one table upload and one materialise launch for all of them."""
    if len(maps) != len(ctxs) or not len(ctxs):
        raise ValueError("map_load_batch: one map per context, at least one")
    lib = ctxs[0]._lib                                          # the build the contexts were created on
    n = len(ctxs)
    ms = (C.c_void_p * n)(*[m.handle for m in maps])
    cs = (_ctx * n)(*[c.handle for c in ctxs])
    r = _dvec(np.asarray(ref_invs, dtype=np.float64), 16 * n)
    st = lib.velo_map_load_batch(ms, cs, n, _ptr(r))
    if st != 0:
        msg = lib.velo_last_error()
        raise VeloError(f"velo status {st}: {msg.decode() if msg else ''}")


def comm_unique_id() -> bytes:
    lib = load_library()
    buf = C.create_string_buffer(128)
    st = lib.velo_comm_unique_id(buf)
    if st != 0:
        raise VeloError(f"velo_comm_unique_id failed: {st}")
    return buf.raw


def frame_to_frame_batch(ctxs, x0s):
    """B independent scan pairs in flight, one context each.  The library advances them in lock-step on one stream with shared LM
    launches when it can (same device and parameters, no communicator, no visual blocks), else with a host thread per context."""
    lib = ctxs[0]._lib if len(ctxs) else load_library()      # the build the contexts were created on
    n = len(ctxs)
    arr = (_ctx * n)(*[c.handle for c in ctxs])
    x = np.ascontiguousarray(np.asarray(x0s, dtype=np.float64).reshape(n, 6)).copy()
    T = np.zeros((n, 16))
    S = (VeloSummary * n)()
    st = lib.velo_frame_to_frame_batch(arr, n, _ptr(x), _ptr(T), S)
    if st != 0:
        msg = lib.velo_last_error()
        raise VeloError(f"velo status {st}: {msg.decode() if msg else ''}")
    return x, T.reshape(n, 4, 4), list(S)


# -- the visual front end of several contexts in one call each (velo_set_images_batch / velo_track_features_batch /
#    velo_detect_features_batch): what Context.set_images / track_features / detect_features do, for n sequences on one GPU ---------
def _batch_lib_and_handles(ctxs):
    if not len(ctxs):
        raise ValueError("a batch call needs at least one context")
    lib = ctxs[0]._lib                                          # the build the contexts were created on
    return lib, (_ctx * len(ctxs))(*[c.handle for c in ctxs])


def _batch_check(lib, st):
    if st != 0:
        msg = lib.velo_last_error()
        raise VeloError(f"velo status {st}: {msg.decode() if msg else ''}")


def set_images_batch(ctxs, imgs_per_ctx):
    """Context.set_images for every context in ONE call: imgs_per_ctx[i] is the list of context i's grayscale images (2-D uint8, one
    shape per context, the same number of cameras for all; shapes may differ between contexts)."""
    lib, arr = _batch_lib_and_handles(ctxs)
    if len(imgs_per_ctx) != len(ctxs):
        raise ValueError("set_images_batch: one image list per context")
    per = [[np.ascontiguousarray(np.asarray(im, dtype=np.uint8)) for im in imgs] for imgs in imgs_per_ctx]
    n_cams = len(per[0])
    if n_cams < 1 or any(len(a) != n_cams for a in per):
        raise ValueError("set_images_batch: the same number of cameras (>= 1) for every context")
    if any(im.ndim != 2 or im.shape != a[0].shape for a in per for im in a):
        raise ValueError("set_images_batch: per context one or more 2-D uint8 images of one shape")
    ptrs = (C.c_void_p * (len(per) * n_cams))(*[im.ctypes.data for a in per for im in a])
    sizes = np.array([[a[0].shape[1], a[0].shape[0], a[0].shape[1]] for a in per], dtype=np.int32)
    _batch_check(lib, lib.velo_set_images_batch(C.cast(arr, C.c_void_p), len(ctxs), C.cast(ptrs, C.c_void_p), n_cams,
                                                C.c_void_p(sizes.ctypes.data)))


def track_features_batch(ctxs, jobs, **params):
    """Every (ctx_index, prev_cam, cam, prev_xy [n, 2] pixels) job in ONE call over all contexts: per job lists of next_xy [n, 2] f32,
    status [n] bool and kept [n] bool, as Context.track_features gives them.  params: lk_params keywords."""
    p = lk_params(**params)
    lib, arr = _batch_lib_and_handles(ctxs)
    pts = [np.ascontiguousarray(np.asarray(xy, dtype=np.float32).reshape(-1, 2)) for _, _, _, xy in jobs]
    jarr = (VeloTrackJob * max(len(jobs), 1))()
    jctx = np.zeros(max(len(jobs), 1), dtype=np.int32)
    for j, ((ci, pc, cc, _), a) in enumerate(zip(jobs, pts)):
        jctx[j] = int(ci)
        jarr[j].prev_cam, jarr[j].cam = int(pc), int(cc)
        jarr[j].prev_xy = a.ctypes.data if len(a) else None
        jarr[j].n = len(a)
    n = int(sum(len(a) for a in pts))
    nxt = np.zeros((max(n, 1), 2), dtype=np.float32)
    st = np.zeros(max(n, 1), dtype=np.uint8)
    kp = np.zeros(max(n, 1), dtype=np.uint8)
    vp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    _batch_check(lib, lib.velo_track_features_batch(C.cast(arr, C.c_void_p), len(ctxs), vp(jctx), C.cast(jarr, C.c_void_p), len(jobs),
                                                    C.byref(p), vp(nxt), vp(st), vp(kp)))
    off = np.concatenate([[0], np.cumsum([len(a) for a in pts])]).astype(np.int64)
    return ([nxt[off[j]:off[j + 1]].copy() for j in range(len(jobs))], [st[off[j]:off[j + 1]].astype(bool) for j in range(len(jobs))],
            [kp[off[j]:off[j + 1]].astype(bool) for j in range(len(jobs))])


def detect_features_batch_raw(ctxs, jobs, capacity: int, xy=None, response=None, fresh=None, **params):
    """velo_detect_features_batch as it is: jobs = [(ctx_index, cam, existing_xy [n, 2] or None)]; returns the caller-sized arrays
    (xy [n_jobs, capacity, 2], response, fresh, counts [n_jobs, 3]); arrays handed in are written in place"""
    p = gftt_params(**params)
    lib, arr = _batch_lib_and_handles(ctxs)
    n_jobs = len(jobs)
    pts = [np.ascontiguousarray(np.asarray(np.zeros((0, 2)) if e is None else e, dtype=np.float32).reshape(-1, 2)) for _, _, e in jobs]
    jarr = (VeloDetectJob * max(n_jobs, 1))()
    jctx = np.zeros(max(n_jobs, 1), dtype=np.int32)
    for j, ((ci, cam, _), a) in enumerate(zip(jobs, pts)):
        jctx[j] = int(ci)
        jarr[j].cam, jarr[j].n_existing = int(cam), len(a)
        jarr[j].existing_xy = a.ctypes.data if len(a) else None
    cap = int(capacity)
    xy = np.zeros((max(n_jobs, 1), max(cap, 1), 2), dtype=np.float32) if xy is None else xy
    response = np.zeros((max(n_jobs, 1), max(cap, 1)), dtype=np.float32) if response is None else response
    fresh = np.zeros((max(n_jobs, 1), max(cap, 1)), dtype=np.uint8) if fresh is None else fresh
    counts = np.zeros((max(n_jobs, 1), 3), dtype=np.int32)
    vp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    _batch_check(lib, lib.velo_detect_features_batch(C.cast(arr, C.c_void_p), len(ctxs), vp(jctx), C.cast(jarr, C.c_void_p), n_jobs,
                                                     C.byref(p), cap, vp(xy), vp(response), vp(fresh), vp(counts)))
    return xy, response, fresh, counts[:n_jobs]


def detect_features_batch(ctxs, jobs, return_counts: bool = False, **params):
    """Every (ctx_index, cam, existing_xy [n, 2] pixels or None) job in ONE call on the current images of the contexts: per job
    (xy [k, 2] f32, response [k] f32, fresh [k] bool) in selection order, as Context.detect_features gives them.  params:
    gftt_params keywords (max_corners, quality_level, min_distance)."""
    p = gftt_params(**params)
    cap = p.max_corners if p.max_corners > 0 else 4096
    while True:
        xy, resp, fr, counts = detect_features_batch_raw(ctxs, jobs, cap, **params)
        need = int(counts[:, 0].max()) if len(jobs) else 0
        if need <= cap:
            break
        cap = need                                  # no cap on the corners and more of them than assumed: once more, sized right
    res = [(xy[j, :counts[j, 0]].copy(), resp[j, :counts[j, 0]].copy(), fr[j, :counts[j, 0]].astype(bool)) for j in range(len(jobs))]
    return (res, counts.copy()) if return_counts else res


def landmarks_triangulate_batch(ctxs, frames, capacity: Optional[int] = None, raw: bool = False):
    """Context.landmarks_triangulate for frames[i] of ctxs[i] in ONE call (one gather launch, one solve launch): per context
    (ids, points, results).  capacity / raw: the call as it is -- context-major arrays ids [n_ctx, capacity], points
    [n_ctx, capacity, 3], results [n_ctx, capacity] and the counts n [n_ctx] (a count above `capacity` means truncated outputs;
    every landmark is solved and stored all the same)."""
    lib, arr = _batch_lib_and_handles(ctxs)
    if len(frames) != len(ctxs):
        raise ValueError("landmarks_triangulate_batch: one frame per context")
    fr = np.ascontiguousarray(np.asarray(frames, dtype=np.int32).reshape(-1))
    n_ctx = len(ctxs)
    if capacity is None:                             # what the largest context of the call will solve: host bookkeeping, no device work
        cap = max(c.landmarks_frame_count(f)[1] for c, f in zip(ctxs, fr))
    else:
        cap = int(capacity)
    if cap < 0:
        raise ValueError("landmarks_triangulate_batch: capacity >= 0")
    ids = np.zeros((n_ctx, max(cap, 1)), dtype=np.int32)
    pts = np.zeros((n_ctx, max(cap, 1), 3), dtype=np.float32)
    res = np.zeros((n_ctx, max(cap, 1)), dtype=TRI_RESULT_DTYPE)
    n = np.zeros(n_ctx, dtype=np.int32)
    vp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    _batch_check(lib, lib.velo_landmarks_triangulate_batch(C.cast(arr, C.c_void_p), n_ctx, vp(fr), vp(ids), vp(pts), vp(res), cap, vp(n)))
    if raw or capacity is not None:
        return ids[:, :cap], pts[:, :cap], res[:, :cap], n
    return [(ids[i, :n[i]].copy(), pts[i, :n[i]].copy(), res[i, :n[i]].copy()) for i in range(n_ctx)]


def build_matches_batch(ctxs, frames1, frames2, poses2_inv=None, capacity: Optional[int] = None, raw: bool = False, _with_cams: bool = False):
    """Context.build_matches for (frames1[i], frames2[i]) of ctxs[i] in ONE call (the same four launches for all): per context
    (n_per_cam, pairs), as the call wrote them.  poses2_inv: one 4 x 4 inverse pose per context, or None (no landmark substitution
    anywhere).  capacity: the pairs every context gets room for (default: the keypoints of the largest frame2, which bounds every
    count; host bookkeeping, no device work).  capacity / raw: the call's arrays as they are -- n_per_cam [n_ctx, 8], pairs
    [n_ctx, capacity, 2] and the counts n [n_ctx] (a count above `capacity` means truncated pairs; the visual set is complete all
    the same)."""
    lib, arr = _batch_lib_and_handles(ctxs)
    n_ctx = len(ctxs)
    if len(frames1) != n_ctx or len(frames2) != n_ctx:
        raise ValueError("build_matches_batch: one frame pair per context")
    f1 = np.ascontiguousarray(np.asarray(frames1, dtype=np.int32).reshape(-1))
    f2 = np.ascontiguousarray(np.asarray(frames2, dtype=np.int32).reshape(-1))
    M = None
    if poses2_inv is not None:
        M = np.ascontiguousarray(np.asarray(poses2_inv, dtype=np.float64).reshape(-1))
        if M.size != 16 * n_ctx:
            raise ValueError("build_matches_batch: one 4 x 4 inverse pose per context")
    vp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    sizes = [c.frames_count(f) for c, f in zip(ctxs, f2)]      # also raises when a context has no frame store
    cap = max(s[1] for s in sizes) if capacity is None else int(capacity)
    per_cam = np.zeros((n_ctx, 8), dtype=np.int32)
    n = np.zeros(n_ctx, dtype=np.int32)
    pairs = np.zeros((n_ctx, max(cap, 1), 2), dtype=np.int32)
    _batch_check(lib, lib.velo_build_matches_batch(C.cast(arr, C.c_void_p), n_ctx, vp(f1), vp(f2), vp(M) if M is not None else None,
                                                   vp(per_cam), vp(pairs), cap, vp(n)))
    n_cams = [len(s[0]) for s in sizes]
    if _with_cams:
        return per_cam, pairs[:, :cap], n, n_cams
    if raw or capacity is not None:
        return per_cam, pairs[:, :cap], n
    return [(per_cam[i, :n_cams[i]].copy(), pairs[i, :n[i]].copy()) for i in range(n_ctx)]


def build_matches_desc_batch(ctxs, frames1, frames2, poses2_inv=None, match_thresh: float = 29.0, capacity: Optional[int] = None,
                             raw: bool = False, _with_cams: bool = False):
    """Context.build_matches_desc for (frames1[i], frames2[i]) of ctxs[i] in ONE call (the same three launches for all); arguments
    and results as build_matches_batch.  capacity defaults to the keypoints of the largest frame1 (the query side), which bounds every
    count."""
    lib, arr = _batch_lib_and_handles(ctxs)
    n_ctx = len(ctxs)
    if len(frames1) != n_ctx or len(frames2) != n_ctx:
        raise ValueError("build_matches_desc_batch: one frame pair per context")
    f1 = np.ascontiguousarray(np.asarray(frames1, dtype=np.int32).reshape(-1))
    f2 = np.ascontiguousarray(np.asarray(frames2, dtype=np.int32).reshape(-1))
    M = None
    if poses2_inv is not None:
        M = np.ascontiguousarray(np.asarray(poses2_inv, dtype=np.float64).reshape(-1))
        if M.size != 16 * n_ctx:
            raise ValueError("build_matches_desc_batch: one 4 x 4 inverse pose per context")
    vp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    sizes = [c.frames_count(f) for c, f in zip(ctxs, f1)]      # also raises when a context has no frame store
    cap = max(s[1] for s in sizes) if capacity is None else int(capacity)
    per_cam = np.zeros((n_ctx, 8), dtype=np.int32)
    n = np.zeros(n_ctx, dtype=np.int32)
    pairs = np.zeros((n_ctx, max(cap, 1), 2), dtype=np.int32)
    _batch_check(lib, lib.velo_build_matches_desc_batch(C.cast(arr, C.c_void_p), n_ctx, vp(f1), vp(f2), vp(M) if M is not None else None,
                                                        float(match_thresh), vp(per_cam), vp(pairs), cap, vp(n)))
    n_cams = [len(s[0]) for s in sizes]
    if _with_cams:
        return per_cam, pairs[:, :cap], n, n_cams
    if raw or capacity is not None:
        return per_cam, pairs[:, :cap], n
    return [(per_cam[i, :n_cams[i]].copy(), pairs[i, :n[i]].copy()) for i in range(n_ctx)]


def frames_prune_batch(ctxs, frames, raw: bool = False):
    """Context.frames_prune for (ctxs[i], frames[i]) in ONE call (the same launches for all): per context (list of the kept old
    indices per camera, n_with_depth [n_cams]).  raw: the call's arrays as they are -- n_kept [n_ctx, 8], n_with_depth [n_ctx, 8],
    kept_out [n_ctx, capacity], n_out [n_ctx]."""
    lib, arr = _batch_lib_and_handles(ctxs)
    n_ctx = len(ctxs)
    if len(frames) != n_ctx:
        raise ValueError("frames_prune_batch: one frame per context")
    f = np.ascontiguousarray(np.asarray(frames, dtype=np.int32).reshape(-1))
    sizes = [c.frames_count(fr) for c, fr in zip(ctxs, f)]     # also raises when a context has no frame store
    cap = max(s[1] for s in sizes)
    n_kept, n_wd = np.zeros((n_ctx, 8), dtype=np.int32), np.zeros((n_ctx, 8), dtype=np.int32)
    kept = np.zeros((n_ctx, max(cap, 1)), dtype=np.int32)
    n = np.zeros(n_ctx, dtype=np.int32)
    vp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    _batch_check(lib, lib.velo_frames_prune_batch(C.cast(arr, C.c_void_p), n_ctx, vp(f), vp(n_kept), vp(n_wd), vp(kept), cap, vp(n)))
    if raw:
        return n_kept, n_wd, kept[:, :cap], n
    out = []
    for i in range(n_ctx):
        n_cams = len(sizes[i][0])
        cuts = np.r_[0, np.cumsum(n_kept[i, :n_cams])]
        out.append(([kept[i, cuts[c]:cuts[c + 1]].copy() for c in range(n_cams)], n_wd[i, :n_cams].copy()))
    return out


def frames_put_frame_batch(ctxs, frames, cams_per_ctx, thresh: float = 0.015, of_target=None, observe: bool = False, raw: bool = False):
    """Context.frames_put_frame for (ctxs[i], frames[i], cams_per_ctx[i]) in ONE call (the same launches for all); of_target: one
    flag per context (None: the source everywhere).  Per context n_with_depth [n_cams] i32; raw: the call's [n_ctx, 8] array."""
    lib, arr = _batch_lib_and_handles(ctxs)
    n_ctx = len(ctxs)
    if len(frames) != n_ctx or len(cams_per_ctx) != n_ctx:
        raise ValueError("frames_put_frame_batch: one frame and one camera list per context")
    f = np.ascontiguousarray(np.asarray(frames, dtype=np.int32).reshape(-1))
    t = np.ascontiguousarray(np.asarray([0] * n_ctx if of_target is None else [int(bool(v)) for v in of_target], dtype=np.int32).reshape(-1))
    if len(t) != n_ctx:
        raise ValueError("frames_put_frame_batch: one of_target flag per context")
    table = (VeloFrameCam * (8 * n_ctx))()
    for i, cams in enumerate(cams_per_ctx):
        if len(cams) > 8:
            raise ValueError("frames_put_frame_batch: at most 8 cameras")
        for k, cam in enumerate(cams):
            table[8 * i + k] = cam.as_struct()
    n_wd = np.zeros((n_ctx, 8), dtype=np.int32)
    vp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
    _batch_check(lib, lib.velo_frames_put_frame_batch(C.cast(arr, C.c_void_p), n_ctx, vp(f), vp(t), C.cast(table, C.c_void_p), float(thresh),
                                                      VELO_PUT_OBSERVE if observe else 0, vp(n_wd)))
    if raw:
        return n_wd
    return [n_wd[i, :len(cams)].copy() for i, cams in enumerate(cams_per_ctx)]


SCAN_ON_DEVICE, SCAN_SHARED, SCAN_PROMOTE = 1, 2, 4


def scan_refs(scans, device=None, shared=False):
    """[(xyz, ring_offsets), ...] -> (velo_scan_ref array, objects to keep alive while it is in use).  xyz: numpy (n,3|4) float32 or a
    torch tensor on the GPU, as for Context.set_target (device: the contexts' device, checked against the tensors').  Device tensors
    must not be written by torch between this call and the registration that uses the descriptors."""
    n = len(scans)
    arr = (VeloScanRef * n)()
    keep = []
    seen = {}                       # the same (cloud, offsets) objects give the same descriptor (what SCAN_SHARED keys on)
    for i, (xyz, off) in enumerate(scans):
        key = (id(xyz), id(off))
        if key not in seen:
            seen[key] = Context._cloud_args(xyz, off, device)
        ptr, stride, off_a, dev, k = seen[key]
        arr[i].xyz = ptr.value
        arr[i].stride_bytes = stride
        arr[i].ring_offsets = off_a.ctypes.data
        arr[i].n_rings = len(off_a) - 1
        arr[i].on_device = dev | (SCAN_SHARED if shared else 0)
        keep.append((k, off_a))
    return arr, keep


def promote_refs(n: int):
    """n target descriptors that say "this job's target is the scan the context holds as its source" (VELO_SCAN_PROMOTE): the step of a
    drive, where frame k -- registered as source in the last call -- is the target of frame k+1 (main.cpp:233,380)."""
    arr = (VeloScanRef * n)()
    for i in range(n):
        arr[i].xyz = None
        arr[i].stride_bytes = 16
        arr[i].ring_offsets = None
        arr[i].n_rings = 0
        arr[i].on_device = SCAN_ON_DEVICE | SCAN_PROMOTE
    return arr, []


def visual_refs(matches_per_job):
    """[matches of job 0, ...] (structured arrays / dicts / None) -> (pointer array, count array, objects to keep alive) for
    register_batch(..., visual=...)."""
    n = len(matches_per_job)
    ptrs = (C.c_void_p * n)()
    cnt = (C.c_int32 * n)()
    keep = []
    for i, m in enumerate(matches_per_job):
        if isinstance(m, dict):
            m = matches_from_dict(m)
        a = np.ascontiguousarray(m, dtype=MATCH_DTYPE) if m is not None else np.zeros(0, MATCH_DTYPE)
        ptrs[i] = a.ctypes.data if len(a) else None
        cnt[i] = len(a)
        keep.append(a)
    return ptrs, cnt, keep


def register_batch(ctxs, targets, sources, x0s, refs=None, visual=None):
    """velo_register_batch: job i's target / source scans go into context i and the batch is registered, all inside the library
    (the index builds run on the threads that drive the groups).  targets / sources: lists of (xyz, ring_offsets) or None to keep
    what the contexts hold; refs = (target_refs, source_refs) from scan_refs() to reuse prepared descriptors across calls;
    visual = visual_refs(...) hands the jobs' matches over in the same call (velo_register_batch_visual)."""
    lib = ctxs[0]._lib if len(ctxs) else load_library()      # the build the contexts were created on
    n = len(ctxs)
    arr = (_ctx * n)(*[c.handle for c in ctxs])
    if refs is None:
        dev = ctxs[0]._device if n else None
        tr = scan_refs(targets, dev) if targets is not None else (None, None)
        sr = scan_refs(sources, dev) if sources is not None else (None, None)
    else:
        tr, sr = refs
    x = np.ascontiguousarray(np.asarray(x0s, dtype=np.float64).reshape(n, 6)).copy()
    T = np.zeros((n, 16))
    S = (VeloSummary * n)()
    tp = C.cast(tr[0], C.c_void_p) if tr[0] is not None else None
    sp = C.cast(sr[0], C.c_void_p) if sr[0] is not None else None
    if visual is not None:
        st = lib.velo_register_batch_visual(arr, n, tp, sp, C.cast(visual[0], C.c_void_p), C.cast(visual[1], C.c_void_p), _ptr(x), _ptr(T), S)
    else:
        st = lib.velo_register_batch(arr, n, tp, sp, _ptr(x), _ptr(T), S)
    if st != 0:
        msg = lib.velo_last_error()
        raise VeloError(f"velo status {st}: {msg.decode() if msg else ''}")
    return x, T.reshape(n, 4, 4), list(S)


def hint_next_sources(ctxs, refs):
    """velo_hint_next_source for every context: refs = scan_refs(...)[0] of the clouds the NEXT call will hand over as sources (host clouds are
    uploaded under the current call's launches; device clouds ignore the hint)."""
    lib = ctxs[0]._lib if len(ctxs) else load_library()
    for i, c in enumerate(ctxs):
        st = lib.velo_hint_next_source(c.handle, C.addressof(refs[i]))
        if st != 0:
            msg = lib.velo_last_error()
            raise VeloError(f"velo status {st}: {msg.decode() if msg else ''}")


def hint_next_frames(ctxs, refs):
    """velo_hint_next_frame for every context: refs = scan_refs(...)[0] of the frames the NEXT call will bring as sources behind a promotion
    (the step of a drive): their loads are enqueued behind the current call's launches."""
    lib = ctxs[0]._lib if len(ctxs) else load_library()
    for i, c in enumerate(ctxs):
        st = lib.velo_hint_next_frame(c.handle, C.addressof(refs[i]))
        if st != 0:
            msg = lib.velo_last_error()
            raise VeloError(f"velo status {st}: {msg.decode() if msg else ''}")


def sequence_refs(frames_per_drive, device=None, first=1, count=None):
    """Descriptors of the frames a register_sequences call walks: frames_per_drive[i] = [(xyz, ring_offsets), ...] of drive i; frames
    first .. first + count - 1 of every drive, laid out [frame][drive] as velo_register_sequences takes them.  -> (array, keep-alive)"""
    n = len(frames_per_drive)
    count = (min(len(f) for f in frames_per_drive) - first) if count is None else count
    flat = [frames_per_drive[i][first + f] for f in range(count) for i in range(n)]
    arr, keep = scan_refs(flat, device)
    return arr, keep, count


def sequence_visual_refs(matches_per_drive, first=0, count=None):
    """matches_per_drive[i][k] = the matches of drive i's pair k (frame k+1 against frame k) -> pointer / count arrays laid out [frame][drive]"""
    n = len(matches_per_drive)
    count = (min(len(m) for m in matches_per_drive) - first) if count is None else count
    return visual_refs([matches_per_drive[i][first + f] for f in range(count) for i in range(n)])


SEQ_LOCKSTEP, SEQ_ANNOUNCE = 1, 2


def register_sequences(ctxs, frame_refs, n_frames, poses, x_guess, visual=None, summaries=True, lockstep=False):
    """velo_register_sequences: the drive loop of len(ctxs) sequences for n_frames frames in one call (every context holds its drive's
    current frame as source).  frame_refs: sequence_refs(...)[0]; poses (n,4,4) and x_guess (n,6) float64 C-contiguous, UPDATED IN PLACE
    (the drives' accumulated poses and the next frame's constant-velocity guesses).  lockstep: the groups start every frame together
    (VELO_SEQ_LOCKSTEP).  -> xs (F,n,6), Ts (F,n,4,4), summaries [F][n] or None"""
    lib = ctxs[0]._lib if len(ctxs) else load_library()
    n = len(ctxs)
    assert poses.dtype == np.float64 and poses.flags.c_contiguous and poses.shape == (n, 4, 4)
    assert x_guess.dtype == np.float64 and x_guess.flags.c_contiguous and x_guess.shape == (n, 6)
    arr = (_ctx * n)(*[c.handle for c in ctxs])
    xs = np.zeros((n_frames, n, 6))
    Ts = np.zeros((n_frames, n, 16))
    S = (VeloSummary * (n * n_frames))() if summaries else None
    vm = C.cast(visual[0], C.c_void_p) if visual is not None else None
    vn = C.cast(visual[1], C.c_void_p) if visual is not None else None
    st = lib.velo_register_sequences(arr, n, n_frames, C.cast(frame_refs, C.c_void_p), vm, vn, _ptr(poses), _ptr(x_guess), _ptr(xs), _ptr(Ts), S,
                                     SEQ_LOCKSTEP if lockstep else 0)
    if st != 0:
        msg = lib.velo_last_error()
        raise VeloError(f"velo status {st}: {msg.decode() if msg else ''}")
    return xs, Ts.reshape(n_frames, n, 4, 4), ([[S[f * n + i] for i in range(n)] for f in range(n_frames)] if summaries else None)


class DriveStep:
    """The step of len(ctxs) drives as ONE C call with every argument prepared once: velo_register_sequences for one frame, the frame after it
    announced (VELO_SEQ_ANNOUNCE) -- promote, load, register, chain the pose, predict the motion (main.cpp:305-413 for n sequences).  What a
    compiled caller's loop body costs on the host; register_batch + pose_handoff build a dozen numpy / ctypes objects per step.
    poses (n,4,4) and x_guess (n,6): float64 C-contiguous, UPDATED IN PLACE by every step."""

    def __init__(self, ctxs, poses, x_guess):
        self._lib = ctxs[0]._lib
        self.n = n = len(ctxs)
        assert poses.dtype == np.float64 and poses.flags.c_contiguous and poses.shape == (n, 4, 4)
        assert x_guess.dtype == np.float64 and x_guess.flags.c_contiguous and x_guess.shape == (n, 6)
        self._keep = (ctxs, poses, x_guess)
        self._arr = (_ctx * n)(*[c.handle for c in ctxs])
        self._pp, self._xg = _ptr(poses), _ptr(x_guess)

    def outputs(self, n_steps):
        """result blocks for n_steps steps, allocated once: (xs (S,n,6), Ts (S,n,4,4), summaries [S] of VeloSummary * n, per-step pointers)"""
        n = self.n
        xs, Ts = np.zeros((n_steps, n, 6)), np.zeros((n_steps, n, 16))
        S = [(VeloSummary * n)() for _ in range(n_steps)]
        ptrs = [(C.cast(xs[k].ctypes.data, _dp), C.cast(Ts[k].ctypes.data, _dp)) for k in range(n_steps)]
        return xs, Ts.reshape(n_steps, n, 4, 4), S, ptrs

    def __call__(self, frames_ptr, out_ptrs, summaries, visual=None, announce=False):
        """frames_ptr: c_void_p of n (announce: 2 n) velo_scan_ref -- this step's frames, then the next step's; out_ptrs / summaries: one step's
        entries of outputs(); visual: (pointer array, count array) cast to c_void_p, or None"""
        st = self._lib.velo_register_sequences(self._arr, self.n, 1, frames_ptr, visual[0] if visual else None, visual[1] if visual else None, self._pp, self._xg,
                                               out_ptrs[0], out_ptrs[1], summaries, SEQ_LOCKSTEP | (SEQ_ANNOUNCE if announce else 0))
        if st != 0:
            msg = self._lib.velo_last_error()
            raise VeloError(f"velo status {st}: {msg.decode() if msg else ''}")


def pose_handoff(poses: np.ndarray, dpose: np.ndarray):
    """velo_pose_handoff: poses (n,4,4) float64 C-contiguous, UPDATED IN PLACE to poses @ dpose (main.cpp:408); returns the (n,6) guesses
    of the next frame, the 6-vectors of poses_old^-1 poses_new (main.cpp:311-331)."""
    lib = load_library()
    assert poses.dtype == np.float64 and poses.flags.c_contiguous and poses.shape[1:] == (4, 4)
    n = poses.shape[0]
    d = np.ascontiguousarray(np.asarray(dpose, dtype=np.float64).reshape(n, 16))
    x = np.zeros((n, 6))
    st = lib.velo_pose_handoff(n, _ptr(poses), _ptr(d), _ptr(x))
    if st != 0:
        msg = lib.velo_last_error()
        raise VeloError(f"velo status {st}: {msg.decode() if msg else ''}")
    return x


def pose_vec_to_mat(x) -> np.ndarray:
    lib = load_library()
    xv = _dvec(x, 6)
    T = np.zeros(16)
    lib.velo_pose_vec_to_mat(_ptr(xv), _ptr(T))
    return T.reshape(4, 4)


def pose_mat_to_vec(T) -> np.ndarray:
    lib = load_library()
    Tv = _dvec(T, 16)
    x = np.zeros(6)
    lib.velo_pose_mat_to_vec(_ptr(Tv), _ptr(x))
    return x


def graph_edge_information(z, JtJ) -> np.ndarray:
    """velo_graph_edge_information: the 6 x 6 information W of the edge a registration makes (a host function: no context, no GPU).
    z: the registration's result (6); JtJ: its 6 x 6 at that result, as evaluate returns it."""
    zz = _dvec(z, 6)
    H = np.ascontiguousarray(np.asarray(JtJ, dtype=np.float64).reshape(36))
    out = np.zeros(21, dtype=np.float64)
    lib = load_library()
    st = lib.velo_graph_edge_information(C.c_void_p(zz.ctypes.data), C.c_void_p(H.ctypes.data), C.c_void_p(out.ctypes.data))
    if st != 0:
        msg = lib.velo_last_error()
        raise VeloError(f"velo status {st}: {msg.decode() if msg else ''}")
    W = np.zeros((6, 6))
    W[np.triu_indices(6)] = out
    return W + np.triu(W, 1).T


def graph_order(n_nodes: int, a, b):
    """velo_graph_order: the reverse Cuthill-McKee order the envelope solver of graph_optimize factors in (a host function: no
    context, no GPU).  Nodes 0 .. n_nodes - 1, edges (a[e], b[e]).  Returns (perm [n] int32: the node at position k, first [n] int32:
    the smallest position among k and its neighbours, stats: dict(widest_row, envelope_blocks, work, components))."""
    lib = load_library()
    ea = np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1))
    eb = np.ascontiguousarray(np.asarray(b, dtype=np.int32).reshape(-1))
    if len(ea) != len(eb):
        raise ValueError("graph_order: one a and one b per edge")
    n = max(int(n_nodes), 0)
    perm, first, stats = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32), np.zeros(4, dtype=np.int64)
    vp = lambda v: C.c_void_p(v.ctypes.data) if v.size else None   # noqa: E731
    st = lib.velo_graph_order(int(n_nodes), len(ea), vp(ea), vp(eb), vp(perm), vp(first), vp(stats))
    if st != 0:
        msg = lib.velo_last_error()
        raise VeloError(f"velo status {st}: {msg.decode() if msg else ''}")
    return perm[:n], first[:n], dict(widest_row=int(stats[0]), envelope_blocks=int(stats[1]), work=int(stats[2]), components=int(stats[3]))


def graph_order_extend(n_old: int, perm_old, n_nodes: int, a, b, first_new_edge: int, max_work: int = 1 << 24):
    """velo_graph_order_extend: the order of a graph that has grown since the order perm_old of its first n_old nodes was kept (a host
    function: no context, no GPU).  a, b: all edges, new from first_new_edge on.  Returns (perm, first, stats: dict(widest_row,
    envelope_blocks, work, components, first_dirty_row, rebuilt, reversed, fresh_work))."""
    lib = load_library()
    po = np.ascontiguousarray(np.asarray(perm_old, dtype=np.int32).reshape(-1))
    ea = np.ascontiguousarray(np.asarray(a, dtype=np.int32).reshape(-1))
    eb = np.ascontiguousarray(np.asarray(b, dtype=np.int32).reshape(-1))
    if len(ea) != len(eb):
        raise ValueError("graph_order_extend: one a and one b per edge")
    if len(po) != int(n_old):
        raise ValueError("graph_order_extend: perm_old has n_old entries")
    n = max(int(n_nodes), 0)
    perm, first, stats = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.int32), np.zeros(8, dtype=np.int64)
    vp = lambda v: C.c_void_p(v.ctypes.data) if v.size else None   # noqa: E731
    st = lib.velo_graph_order_extend(int(n_old), vp(po), int(n_nodes), len(ea), vp(ea), vp(eb), int(first_new_edge), int(max_work), vp(perm), vp(first), vp(stats))
    if st != 0:
        msg = lib.velo_last_error()
        raise VeloError(f"velo status {st}: {msg.decode() if msg else ''}")
    keys = ("widest_row", "envelope_blocks", "work", "components", "first_dirty_row", "rebuilt", "reversed", "fresh_work")
    return perm[:n], first[:n], {k: int(stats[i]) for i, k in enumerate(keys)}
