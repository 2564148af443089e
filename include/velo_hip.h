/*
 * velo_hip.h -- C-ABI of the MI355X (gfx950) scan-matching core.
 *
 * This is the drop-in boundary for ONE path of lichunshang/vision-enhanced-lidar-odometry (VELO):
 * the frame-to-frame registration loop  frameToFrame()  (reference velo.h:598-919).  The reference has
 * no FFI/plugin interface; the three de-facto seams the path sits behind are
 *     (1) frameToFrame(...)                     velo.h:598-614, sole caller main.cpp:388-405
 *     (2) the residual functors                 costfunctions.h:17-220
 *     (3) ceres::CostFunction::Evaluate [3P]    used at velo.h:683-689,710-718,744-752,777-785,875-891
 * Each entry point below names the reference lines it replaces.  include/velo_frame_to_frame.hpp is the
 * header-only C++ adaptor that offers seam (1)'s parameter list on top of these calls; INTEGRATION.md
 * shows the binding a maintainer of the reference would add.
 *
 * Conventions: plain pointers and sizes only; every call returns an int status (VELO_OK == 0, < 0 error)
 * and never throws; the caller owns host buffers, the context owns device buffers; one context per host
 * thread (a context is not internally thread-safe), several contexts may share one GPU.
 * x = (omega[3], t[3]) is the reference's `double transform[6]` (velo.h:610): p_prev = R(omega) p_cur + t.
 *
 * Environment: the library reads exactly five variables, at velo_create / at the first batch call; none of them changes a result
 * (every setting gives bit-identical poses, tables and summaries; tests/test_gpu_parity.py compares them):
 *     VELO_CHAIN=0           frame_to_frame with a host round trip after every solve instead of one chain of launches per call
 *     VELO_CHAIN_MARGIN=n    LM launches enqueued per solve beyond the previous call's count (default: 1..3 from the recent history)
 *     VELO_BATCH_LOCKSTEP=0  velo_frame_to_frame_batch / velo_register_batch with one host thread per context instead of lock-step groups
 *     VELO_BATCH_GROUPS=n    number of lock-step groups of a batch (default: by batch size, at most 4)
 *     VELO_SPIN=1            hipDeviceScheduleSpin for the calling process
 * The reference's own knobs are compile-time constants (kitti.h:3-35) and arrive through velo_params.  Kernel variants, grid shapes and
 * diagnostics are NOT an environment surface of this library: they exist only in the tools' build (-DVELO_DIAGNOSTICS,
 * libvelo_hip_diag.so; tools/README.md), which the variant parity tests and the dev tools load explicitly.
 */
#ifndef VELO_HIP_H_
#define VELO_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VELO_OK 0
#define VELO_ERR_INVALID (-1)   /* bad argument (NULL, negative size, empty ring, ...) */
#define VELO_ERR_HIP (-2)       /* a HIP runtime call failed; velo_last_error() has the text */
#define VELO_ERR_STATE (-3)     /* call order violated (e.g. associate before set_target) */
#define VELO_ERR_COMM (-4)      /* RCCL failure */
#define VELO_ERR_NODEVICE (-5)  /* no gfx950 device visible: the product path has NO CPU fallback */

/* residual_type values, same order as the reference enum ResidualType (velo.h:3-8) */
#define VELO_RESIDUAL_3D3D 0
#define VELO_RESIDUAL_3D2D 1
#define VELO_RESIDUAL_2D3D 2
#define VELO_RESIDUAL_2D2D 3
/* velo_functor.kind only: the ICP functor cost3DPD (costfunctions.h:17-55), which has no ResidualType value */
#define VELO_FUNCTOR_3DPD 4

/* ceres::TerminationType [3P] for one LM solve (velo.h:902) */
#define VELO_CONVERGENCE 0
#define VELO_NO_CONVERGENCE 1
#define VELO_FAILURE 2

#define VELO_MAX_SOLVES 64

/* Every tunable of the path.  Defaults = the reference's compile-time constants (kitti.h:8-10,20-32,
 * main.cpp:43-45) and the Ceres defaults the reference leaves untouched at velo.h:897-902. */
typedef struct velo_params {
    int32_t icp_skip;              /* kitti.h:8   200 (BASELINE configs 2-5 use 1) */
    int32_t f2f_iterations;        /* kitti.h:9   2 */
    int32_t icp_iterations;        /* kitti.h:10  3 */
    int32_t enable_icp;            /* velo.h:613,806; caller passes true (main.cpp:404) */
    int32_t enable_2d2d;           /* main.cpp:44 ENABLE_2D2D (defined) */
    int32_t enable_3d2d;           /* main.cpp:45 ENABLE_3D2D (defined) */
    int32_t max_num_iterations;    /* ceres default 50 */
    int32_t max_consecutive_invalid_steps; /* ceres default 5 */
    double weight_3D2D;            /* kitti.h:20  10 */
    double weight_2D2D;            /* kitti.h:21  500 */
    double weight_3DPD;            /* kitti.h:22  1 */
    double loss_thresh_3D2D;       /* kitti.h:23  0.01 */
    double loss_thresh_2D2D;       /* kitti.h:24  2e-5 */
    double loss_thresh_3DPD;       /* kitti.h:25  0.1 */
    double loss_thresh_3D3D;       /* kitti.h:26  0.04 */
    double outlier_reject;         /* kitti.h:30  5 */
    double correspondence_thresh_icp; /* kitti.h:31  0.5 (a SQUARED distance, velo.h:829) */
    double icp_norm_condition;     /* kitti.h:32  1e-5 */
    double function_tolerance;     /* ceres default 1e-6 */
    double gradient_tolerance;     /* ceres default 1e-10 */
    double parameter_tolerance;    /* ceres default 1e-8 */
    double initial_trust_region_radius; /* 1e4 */
    double max_trust_region_radius;     /* 1e16 */
    double min_trust_region_radius;     /* 1e-32 */
    double min_relative_decrease;       /* 1e-3 */
    double min_lm_diagonal;             /* 1e-6 */
    double max_lm_diagonal;             /* 1e32 */
} velo_params;

/* What velo.h:627-654 gathers for one feature match before it chooses residual types. */
typedef struct velo_match {
    float p3_1[3];   /* 3-D keypoint, frame1 (current), camera-0 frame     velo.h:650 */
    float p3_2[3];   /* 3-D keypoint or landmark, frame2 (previous)        velo.h:634-648 */
    float p2_1[2];   /* canonical 2-D observation in frame1                velo.h:653 */
    float p2_2[2];   /* canonical 2-D observation in frame2                velo.h:654 */
    float t_cam[3];  /* cam_trans[cam]                                     kitti.h:76-78 */
    int32_t cam;
    int32_t point1;  /* passed through into good_matches                   velo.h:628 */
    int32_t point2;  /*                                                    velo.h:629 */
    uint8_t d1;      /* has_depth in frame1                                velo.h:631 */
    uint8_t d2;      /* has_depth in frame2 or landmark                    velo.h:632,644 */
    uint8_t pad[2];
} velo_match;

/* One entry of good_matches[cam] / residual_type[cam] (velo.h:691-692,719-720,754-755,787-788). */
typedef struct velo_good_match {
    int32_t cam;
    int32_t point1;
    int32_t point2;
    int32_t residual_type;
} velo_good_match;

/* One point-to-plane correspondence as the association loop builds it (velo.h:822-874). */
typedef struct velo_corr {
    int32_t valid;       /* 0 = skipped by one of the `continue`s at velo.h:849-851,873 */
    int32_t ring_i;      /* np_s_i */
    int32_t idx_i;       /* np_i   */
    int32_t ring_j;      /* np_s_j */
    int32_t idx_j;       /* np_j   */
    int32_t idx_k;       /* np_k   */
    int32_t src_ring;    /* sm  */
    int32_t src_idx;     /* smi */
    float dist_i;        /* np_dist_i (squared, float) */
    float dist_j;        /* np_dist_j */
    float p[3];          /* pointM_untransformed  velo.h:809 */
    float n[3];          /* N                     velo.h:872-874 */
    float v0[3];         /* v0                    velo.h:869 */
} velo_corr;

/* Target-sharded mode (BASELINE config 5): what one rank knows about a query after searching ONLY the
 * whole target rings it holds.  Ring ownership is disjoint, so the query's owner merges `world` such records with
 * best1 = min key1, best2 = min(key1 of the other ranks, key2 of the winner) and builds the plane from the payload. */
typedef struct velo_partial {
    uint64_t key1, key2;   /* (float bits of d^2) << 32 | global ring-major point index; "absent" compares above every real key */
    int32_t ring1, ring2;  /* global ring ids, -1 when absent */
    int32_t idx1;          /* np_i   (index inside ring1) */
    int32_t idx_k;         /* np_k   (ring neighbour of np_i, velo.h:852-863) */
    int32_t idx2;          /* np_j   (index inside ring2) */
    int32_t pad;
    float v0[3];           /* scans_S[ring1][idx1] */
    float v2[3];           /* scans_S[ring1][idx_k] */
    float v1[3];           /* scans_S[ring2][idx2] */
    float pad2;
} velo_partial;

typedef struct velo_solve_summary {
    int32_t termination;       /* VELO_CONVERGENCE / NO_CONVERGENCE / FAILURE */
    int32_t lm_iterations;     /* trust-region iterations, successful or not */
    int32_t evaluations;       /* residual(+Jacobian) sweeps over all blocks */
    int32_t n_icp_valid;       /* point-to-plane blocks in this solve */
    int32_t n_visual_blocks;   /* visual residual blocks in this solve */
    int32_t n_visual_residuals;
    double initial_cost;
    double final_cost;
} velo_solve_summary;

/* --- "next" row 4 of SURVEY.md 8(f): batched triangulatePoint (velo.h:1027-1130) ------------------------------ */
#define VELO_TRI_OBS_3D 0   /* triangulation3D (costfunctions.h:338-375), TrivialLoss (velo.h:1078) */
#define VELO_TRI_OBS_2D 1   /* triangulation2D (costfunctions.h:288-336), ScaledLoss(CauchyLoss(loss_thresh_3D2D), weight_3D2D) (velo.h:1116-1119) */
typedef struct velo_tri_obs {  /* one entry of keypoint_obs3[cam] / keypoint_obs2[cam] of one landmark: 24 bytes */
    int32_t kind;              /* VELO_TRI_OBS_3D / VELO_TRI_OBS_2D */
    int32_t frame;             /* the map key: index into camera_poses */
    int32_t cam;               /* camera; a 2-D observation uses cam_trans[cam] */
    float s[3];                /* 3-D: the observed point (camera-0 frame of `frame`); 2-D: canonical (x, y), s[2] unused */
} velo_tri_obs;
typedef struct velo_tri_result {   /* per landmark, optional: 24 bytes */
    int32_t n_solves;          /* ceres::Solve calls the reference makes for it: 0 (no observation), 1 or 2 (velo.h:1080-1083,1123) */
    int32_t termination;       /* of the last solve */
    int32_t lm_iterations;     /* of the last solve */
    int32_t evaluations;       /* over all solves */
    double final_cost;
} velo_tri_result;

/* residualStats (velo.h:921-1025): what the reference prints after every f2f iteration (velo.h:909) -- per residual type the
 * median (sorted[size / 2]), mean and count of the block norms at the current pose, loss functions NOT applied
 * (3D3D: |r|_2 of 3; 3D2D / 2D3D: |r|_2 of 2; 2D2D, 3DPD: |r|), plus the cost 1/2 sum r^2 of that evaluation.
 * type[k]: k = VELO_RESIDUAL_3D3D, _3D2D, _2D3D, _2D2D, VELO_FUNCTOR_3DPD.  Computed on the device (radix select, no sort). */
typedef struct velo_residual_stat { double median, mean; int64_t count; } velo_residual_stat;
typedef struct velo_residual_stats {
    velo_residual_stat type[5];
    double cost;
    int32_t n_blocks, n_residuals;     /* problem.NumResidualBlocks(), problem.NumResiduals() */
} velo_residual_stats;                 /* 136 bytes */
#define VELO_MAX_STATS 4               /* f2f iterations whose statistics a summary keeps */

typedef struct velo_summary {
    int32_t n_solves;
    int32_t n_assoc_rounds;
    int32_t n_queries;                 /* Nq per round */
    int32_t n_target;                  /* Nt */
    uint64_t algorithmic_bytes;        /* sum B_assoc + sum B_eval */
    uint64_t assoc_bytes;              /* the B_assoc part */
    double assoc_kernel_ms;            /* sum of association-search launch durations (HIP events) when timing is on */
    int32_t assoc_kernel_launches;
    int32_t eval_kernel_launches;
    double eval_kernel_ms;
    velo_solve_summary solves[VELO_MAX_SOLVES];
    int32_t n_residual_stats;          /* f2f iterations recorded below (0 unless velo_set_residual_stats(ctx, 1)) */
    int32_t reserved;
    velo_residual_stats residual_stats[VELO_MAX_STATS];   /* [iter - 1]: residualStats at the end of f2f iteration iter */
} velo_summary;

typedef struct velo_ctx velo_ctx;

/* --- lifetime ------------------------------------------------------------------------------------ */
/* Binds a context (device buffers + one HIP stream) to `device`.  Replaces cv::cuda::setDevice (main.cpp:64)
 * as the device selection of the path.  Fails with VELO_ERR_NODEVICE when no GPU is visible. */
int velo_create(velo_ctx** out, int device);
int velo_destroy(velo_ctx* ctx);
const char* velo_last_error(void);
const char* velo_version(void);

/* --- configuration: kitti.h:8-10,20-32 + ceres::Solver::Options defaults (velo.h:897-901) ----------- */
int velo_default_params(velo_params* p);
int velo_set_params(velo_ctx* ctx, const velo_params* p);
int velo_get_params(const velo_ctx* ctx, velo_params* p);
/* Launch timing with HIP events (off by default).  enable = 1: the association launches of a call, summed into
 * velo_summary::assoc_kernel_ms.  enable = 2: every instrumented launch -- association, seeds, LM (sweep + step), target index build -- is
 * COUNTED per kernel name, and every 8th launch of a name is bracketed by the kernel's own start / stop events (hipExtLaunchKernelGGL;
 * a bracket costs ~5 us of queue time, so bracketing every launch -- enable = 3 -- slows a chain of 20-us launches by a quarter).  The
 * brackets are read after the call's final synchronisation and accumulated until velo_get_kernel_times collects them: `ms` = bracketed
 * time scaled by launches / sampled (what bench.py's `kernels` list reports).  algorithmic_bytes: SURVEY.md 8(d)'s figure for the
 * launches of that kernel -- B_assoc per association round served, B_eval per LM evaluation -- and, for the index-build and seed kernels,
 * what the kernel must move given the data layout.  Launches shared by the contexts of a lock-step group are logged on the group's
 * first context.  (At levels 2 and 3 the association launches are bracketed one by one, as at level 1.) */
int velo_set_timing(velo_ctx* ctx, int enable);
typedef struct velo_kernel_time {
    char name[48];
    double ms;                         /* estimated sum of launch durations: bracketed time x launches / sampled */
    int64_t launches;
    int64_t sampled;                   /* launches that were bracketed */
    uint64_t algorithmic_bytes;
} velo_kernel_time;                    /* 80 bytes */
int velo_get_kernel_times(velo_ctx* ctx, velo_kernel_time* out, int32_t capacity, int32_t* n, int32_t reset);
/* residualStats after every f2f iteration (velo.h:909) into velo_summary::residual_stats (off by default: the reference only
 * prints them; switched on, a call evaluates between the iterations and is therefore driven round by round from the host). */
int velo_set_residual_stats(velo_ctx* ctx, int enable);

/* --- inputs --------------------------------------------------------------------------------------- */
/* Target = frame2 rings.  Replaces `scans_S` + `kd_trees` (velo.h:606-607) and the per-ring
 * KdTreeFLANN::setInputCloud of ScanData (lru.h:17-20): the spatial index is built on the device here.
 * xyz: first float of point 0; stride_bytes between points (12 packed, 16 for pcl::PointXYZ);
 * ring_offsets[n_rings+1]: ring r = points [ring_offsets[r], ring_offsets[r+1]), each ring an ordered cyclic
 * polyline (kitti.h:158-183).  on_device != 0: xyz is already a device pointer (stays caller-owned, copied).
 * Device pointers (every entry point with an on_device flag, velo_scan_ref included): the memory must be on the context's
 * device, float32, the three coordinates of a point contiguous, and COMPLETE before the call -- the library reads it on the
 * context's own non-blocking stream, which is not ordered against the stream that produced the data: synchronise that
 * stream (or wait for its event) first, and do not overwrite the buffer until the call has returned. */
int velo_set_target(velo_ctx* ctx, const float* xyz, int64_t stride_bytes, const int32_t* ring_offsets,
                    int32_t n_rings, int on_device);
/* Target-sharded variant: this context holds only `n_rings` WHOLE rings of the target (keeps the +-1 ring neighbour of
 * velo.h:852-856 local); `first_ring` is the global id of the first of them and `first_point` the global ring-major index of
 * its first point.  ring_offsets are local ([0] == 0).  velo_set_target == velo_set_target_part(..., 0, 0, ...). */
int velo_set_target_part(velo_ctx* ctx, const float* xyz, int64_t stride_bytes, const int32_t* ring_offsets,
                         int32_t n_rings, int32_t first_ring, int32_t first_point, int on_device);
/* Source = frame1 rings (`scans_M`, velo.h:605).  Queries are every icp_skip-th point of each ring (velo.h:807). */
int velo_set_source(velo_ctx* ctx, const float* xyz, int64_t stride_bytes, const int32_t* ring_offsets,
                    int32_t n_rings, int on_device);
/* "Next" row 1 of SURVEY.md 8(f): the step immediately before the path, on the device.  Replaces loadPoints + segmentPoints
 * (kitti.h:121-185) for one frame: `xyzr` are raw Velodyne records in FILE order (x, y, z, reflectance -> stride 16 for a
 * KITTI .bin), a new ring starts where x > 0 and the sign of y flips (kitti.h:166), points are stored in the camera-0 frame
 * (velo_to_cam: row-major 4x4, float arithmetic like pcl::transformPointCloud) and every ring is reordered
 * new[i] = old[n-1-((i + n/2) % n)] (kitti.h:180).  The result becomes this context's source (as_target == 0) or target. */
int velo_set_scan_velodyne(velo_ctx* ctx, int32_t as_target, const float* xyzr, int64_t stride_bytes, int32_t n_points,
                           const float velo_to_cam[16], int on_device);
/* The scan cache of the odometry loop (replaces the ScansLRU look-up of the previous frame, lru.h:31-61, main.cpp:233,380): the cloud
 * this context holds as SOURCE (frame k, already segmented on the device) becomes its TARGET for the next registration -- device
 * buffers are swapped, nothing is uploaded or segmented again; only the target index (ring ids, grid) is built.  Afterwards the
 * context has no source until the next velo_set_source / velo_set_scan_velodyne(as_target = 0). */
int velo_source_to_target(velo_ctx* ctx);
/* Scan-to-map batches (BASELINE configs 4-5: many scans against ONE accumulated map): `dst` takes the target `src` holds -- cloud
 * and search index -- BY REFERENCE: no copy, no second index build, one 110 MB map in HBM instead of one per context.  The shared
 * target is read-only; it lives as long as any context holds it, and a context that loads a new target simply lets go of it.
 * Both contexts must be on the same device and work with the same gates. */
int velo_share_target(velo_ctx* dst, velo_ctx* src);
/* Device-resident scan cache: the ScansLRU of the reference (lru.h:31-61, `size = 50`; look-ups main.cpp:216,349-350,544) with the
 * scans kept in HBM instead of host memory -- the cloud as the path stores it (camera-0 frame, ring-major) and, for scans stored from
 * a context's TARGET side, the search index built for it (the role of ScanData::trees, lru.h:9,17-20), so a frame that is matched again
 * (frame - dframe for every dframe, main.cpp:306-350) is neither read, segmented, uploaded nor indexed a second time.
 * store: device-to-device copy of the scan a context holds (of_target: its target incl. index / its source) under `frame`; a frame that
 *        is already cached is replaced; the least recently used entry is dropped beyond `capacity` (lru.h:52-57).
 * load:  device-to-device copy into a context as its target or source, and the entry becomes the most recent one (lru.h:42-47).
 *        Loading as target reuses the cached index when it was built for the same gates, otherwise (entries stored from a source,
 *        other params) the index is built from the cached cloud.  Any number of contexts may load the same entry.
 * VELO_ERR_STATE when `frame` is not cached (the caller then reads the scan and stores it: what lru.h:48-58 does).
 * Like a context, a cache is not internally thread-safe: one call at a time (the reference's loop is single-threaded, velo.h:900). */
typedef struct velo_scan_cache velo_scan_cache;
int velo_cache_create(velo_scan_cache** out, int32_t device, int32_t capacity);
int velo_cache_destroy(velo_scan_cache* cache);
int velo_cache_store(velo_scan_cache* cache, int32_t frame, velo_ctx* ctx, int32_t of_target);
int velo_cache_load(velo_scan_cache* cache, int32_t frame, velo_ctx* ctx, int32_t as_target);
int velo_cache_contains(const velo_scan_cache* cache, int32_t frame);                      /* 1 / 0 */
/* frames from most to least recently used; returns the number of cached scans */
int velo_cache_frames(const velo_scan_cache* cache, int32_t* frames_out, int32_t capacity);
/* ring offsets / camera-frame points the context currently holds (for callers that segmented on the device) */
int velo_get_ring_offsets(velo_ctx* ctx, int32_t of_target, int32_t* out, int32_t capacity, int32_t* n_rings);
int velo_get_cloud(velo_ctx* ctx, int32_t of_target, float* xyz_out, int32_t capacity_points, int32_t* n_points);
/* Visual matches of both cameras, in the reference's iteration order cam-major (velo.h:622-627). n may be 0. */
int velo_set_visual(velo_ctx* ctx, const velo_match* matches, int32_t n);

/* --- the pieces (each also usable on its own; tests call them one by one) ---------------------------- */
/* One association round at pose x with the gate of outer iteration `iter` (1-based): velo.h:806-874.
 * Leaves the correspondence table on the device for velo_evaluate / velo_solve. */
int velo_associate(velo_ctx* ctx, const double x[6], int32_t iter, int32_t* n_valid);
/* Target-sharded pieces (tests drive them one by one; with a communicator in target-sharded mode velo_associate runs
 * them as  partial search -> all-to-all of the record slices -> merge  internally):
 *   velo_associate_partial: ALL queries against the local rings, one velo_partial per query left on the device;
 *   velo_get_partials:      copy them to the host;
 *   velo_merge_partials:    merge `world` host tables (each n_queries records) for THIS context's query share into its
 *                           correspondence table (rows A3-A6 finished by the query's owner). */
int velo_associate_partial(velo_ctx* ctx, const double x[6], int32_t iter);
int velo_get_partials(velo_ctx* ctx, velo_partial* out, int32_t capacity, int32_t* n_queries);
int velo_merge_partials(velo_ctx* ctx, const velo_partial* const* tables, int32_t world, int32_t* n_valid);
/* Copies the table back (one record per query, in query order sm-major / smi ascending). */
int velo_get_correspondences(velo_ctx* ctx, velo_corr* out, int32_t capacity, int32_t* n_queries);
/* Visual block selection + outlier gate G1 at pose x: velo.h:622-792. */
int velo_build_visual(velo_ctx* ctx, const double x[6], int32_t iter, int32_t* n_blocks);
int velo_get_good_matches(velo_ctx* ctx, velo_good_match* out, int32_t capacity, int32_t* n);
/* Robustified cost + normal equations of all current blocks at x: what one Ceres evaluation produces
 * (functors costfunctions.h:39-54,76-87,111-126,151-168,192-216; losses velo.h:688,714-717,748-751,
 * 781-784,887-890).  JtJ is the full symmetric 6x6 row-major, Jtr = J^T r, cost = sum 1/2 rho(s). */
int velo_evaluate(velo_ctx* ctx, const double x[6], double* cost, double JtJ[36], double Jtr[6]);
/* Optional row-level output for a ceres::CostFunction adaptor (seam 3): residuals[n_res] and row-major
 * jacobian[n_res*6], robustifier already applied.  Order: visual blocks, then ICP blocks (velo.h order). */
int velo_evaluate_rows(velo_ctx* ctx, const double x[6], double* residuals, double* jacobian,
                       int32_t capacity_rows, int32_t* n_rows);
/* Seam 2 (the functor concept, costfunctions.h:17-220: `template<class T> bool operator()(const T* x, T* residual) const`
 * instantiated by ceres::AutoDiffCostFunction<F, dim, 6>) by value: n functors at one pose in one launch.
 * kind = VELO_RESIDUAL_* or VELO_FUNCTOR_3DPD; c = the functor's constructor arguments widened to double, in the reference's
 * order: cost3D3D m(3) s(3) (costfunctions.h:62-74) | cost3D2D m(3) s(2) t(3) (94-110) | cost2D3D m(3) s(2) t(3) (134-150)
 * | cost2D2D m(2) s(2) t(3) (176-190) | cost3DPD point(3) normal(3) offset(3) (19-37).
 * residuals: n x 3 doubles (rows beyond the functor's dimension are 0), the RAW residuals -- no loss applied;
 * jacobians: n x 18 doubles, row-major dim x 6 per functor = what autodiff returns (may be NULL). */
typedef struct velo_functor {
    int32_t kind;
    int32_t reserved;
    double c[9];
} velo_functor;   /* 80 bytes */
int velo_evaluate_functors(velo_ctx* ctx, const velo_functor* functors, int32_t n, const double x[6],
                           double* residuals, double* jacobians);
/* residualStats (velo.h:921-1025) of the current blocks at x. */
int velo_residual_stats_at(velo_ctx* ctx, const double x[6], velo_residual_stats* out);
/* One ceres::Solve (velo.h:897-902) on the current blocks, x in/out. */
int velo_solve(velo_ctx* ctx, double x[6], velo_solve_summary* summary);

/* --- the path -------------------------------------------------------------------------------------- */
/* frameToFrame (velo.h:598-919): f2f_iterations x [visual blocks; icp_iterations x (associate; solve)].
 * x: in = initial guess, out = solution.  T: 4x4 row-major of the solution (util::pose_mat2vec, utility.h:67-82). */
int velo_frame_to_frame(velo_ctx* ctx, double x[6], double T[16], velo_summary* summary);
/* How the calls above ran.  A single-GPU, LiDAR-only call is enqueued as ONE chain of launches with one host synchronisation at its
 * end: the pose of round r+1's association and every solve's summary stay on the device, and the number of LM launches per solve is
 * the previous call's count plus a margin.  A solve that needs more is detected on the device (the next association finds its pose
 * record not ready); the call is then repeated with a host round trip per solve -- same kernels, bit-identical results.
 * calls = calls that went down the chain, misses = calls that had to be repeated.  VELO_CHAIN=0 (read by velo_create) switches the
 * chain off, VELO_CHAIN_MARGIN=n sets the margin (default 2). */
int velo_chain_stats(const velo_ctx* ctx, int32_t* calls, int32_t* misses);
/* Several independent scan pairs in flight, one context each (what run.fish:2 does with one process per sequence): equivalent
 * to n velo_frame_to_frame calls, results bit-identical.  Contexts on one device are advanced in lock-step groups (one sweep /
 * LM-step launch serves a whole group), otherwise one host thread per context.  Every context may appear once (VELO_ERR_INVALID
 * for duplicates or null entries); the first failing context's status is returned. */
int velo_frame_to_frame_batch(velo_ctx** ctxs, int32_t n, double* x /* n*6 */, double* T /* n*16 */,
                              velo_summary* summaries /* n or NULL */);
/* The same with the scans of every job handed over in the call (seam 1 takes scans_M / scans_S per call, velo.h:606-607): job i's
 * target and source go into context i exactly as velo_set_target / velo_set_source would put them, on the thread that then
 * drives that context's group -- a group starts registering as soon as ITS scans are indexed, no barrier across the batch.
 * targets / sources may be NULL (keep what the contexts hold).  n == 1 is velo_set_target + velo_set_source + velo_frame_to_frame
 * in one call (the single-pair path: one chain of launches, one host synchronisation).  A target loaded here for n >= 2 is indexed
 * with at most 2^24 cells instead of 2^25 (only a 2M-point map reaches either; any cell size gives the same results). */
#define VELO_SCAN_ON_DEVICE 1   /* xyz is a device pointer */
#define VELO_SCAN_SHARED 2      /* targets only: jobs with IDENTICAL descriptors carrying this flag share one device copy and one
                                 * index (scan-to-map: many scans against one map) -- built once, held by reference */
#define VELO_SCAN_PROMOTE 4     /* targets only: this job's target is the scan the context holds as its SOURCE (velo_source_to_target:
                                 * the previous frame of a drive becomes sd_prev, main.cpp:233,380 -- buffer swap + index build, no
                                 * upload, no second segmentation); xyz / ring_offsets of the descriptor are ignored.  The job's source
                                 * descriptor then brings the new frame. */
typedef struct velo_scan_ref {
    const float* xyz;
    int64_t stride_bytes;
    const int32_t* ring_offsets;
    int32_t n_rings;
    int32_t on_device;          /* VELO_SCAN_* flags */
} velo_scan_ref;   /* 32 bytes */
int velo_register_batch(velo_ctx** ctxs, int32_t n, const velo_scan_ref* targets, const velo_scan_ref* sources,
                        double* x /* n*6 */, double* T /* n*16 */, velo_summary* summaries /* n */);
/* The same with the jobs' visual matches handed over in the call as well (seam 1 takes `matches` / `keypoints` per call, velo.h:599-605):
 * job i's n_matches[i] records go into context i as velo_set_visual would put them (0: the context registers LiDAR-only), without a
 * host synchronisation per context -- the step of a tightly-coupled drive (BASELINE configs[2]) is ONE call. */
int velo_register_batch_visual(velo_ctx** ctxs, int32_t n, const velo_scan_ref* targets, const velo_scan_ref* sources,
                               const velo_match* const* matches /* n pointers */, const int32_t* n_matches /* n */,
                               double* x /* n*6 */, double* T /* n*16 */, velo_summary* summaries /* n or NULL */);
/* The drive loop of n sequences for n_frames frames in ONE call -- main.cpp:207-413 (the per-frame loop: load the frame, predict the motion
 * main.cpp:311-331, frameToFrame main.cpp:388-405, chain the pose main.cpp:408) for n sequences at a time; the reference runs sequences as
 * independent processes (run.fish:2).  Context i holds the frame its drive starts from as SOURCE (velo_set_source, or the last frame of an
 * earlier call).  For f = 0 .. n_frames-1: that frame is promoted to target (VELO_SCAN_PROMOTE), frames[f * n + i] is loaded as the new
 * source (with matches[f * n + i] / n_matches[f * n + i] when given), the pair is registered from x_guess[i], x_out / T_out / summaries
 * [f * n + i] receive what velo_register_batch returns for it, and poses[i] / x_guess[i] are handed over exactly as velo_pose_handoff
 * does it.  The lock-step groups walk their drives' frames independently (no barrier across the batch between frames); per pair the
 * results are bit-identical to the frame-by-frame calls.  poses: n 4x4 row-major in/out; x_guess: n*6 in/out (the start-up guess
 * {0,0,0,0,0,1}, main.cpp:170, for a drive's first pair).  flags: VELO_SEQ_LOCKSTEP -- the groups start every frame together (a barrier
 * between frames: the timing of one velo_register_batch call per frame, without the caller in the loop); 0 -- no barrier.
 * VELO_SEQ_ANNOUNCE -- `frames` holds ONE MORE frame per sequence, frames[n_frames * n + i], which is not registered but announced
 * (velo_hint_next_frame): its loads run behind the last frame's launches, and the next call, which must start with exactly that frame,
 * finds it in place.  A caller that gets its frames one at a time makes the step of a drive ONE call this way: n_frames = 1 with the frame
 * after it announced -- load, register, chain the pose, predict the motion (main.cpp:305-413 for n sequences). */
#define VELO_SEQ_LOCKSTEP 1
#define VELO_SEQ_ANNOUNCE 2
int velo_register_sequences(velo_ctx** ctxs, int32_t n, int32_t n_frames, const velo_scan_ref* frames /* n_frames*n (+ n with VELO_SEQ_ANNOUNCE) */,
                            const velo_match* const* matches /* n_frames*n or NULL */, const int32_t* n_matches /* n_frames*n or NULL */,
                            double* poses /* n*16 */, double* x_guess /* n*6 */, double* x_out /* n_frames*n*6 */, double* T_out /* n_frames*n*16 or NULL */,
                            velo_summary* summaries /* n_frames*n or NULL */, int32_t flags);
/* main.cpp:216,349 load a scan per frame.  A caller that knows which HOST cloud it will hand over as the context's NEXT source announces it
 * here; the library uploads it on a copy stream of its own while the current registration's launches run (the upload is issued by the
 * thread that is about to wait for them), and the very next velo_set_source / batch job / sequence frame that names the same pointer and
 * size takes the uploaded copy instead of uploading again.  A different source drops the hint; device clouds ignore it; results never
 * change.  velo_register_sequences does this by itself for the frames it is given. */
int velo_hint_next_source(velo_ctx* ctx, const velo_scan_ref* next);
/* The whole next STEP of a drive announced one call ahead (main.cpp:216,233,349,380): the next job on this context will promote its source
 * (VELO_SCAN_PROMOTE) and bring `next` as the new source.  A chained registration (velo_register_batch[_visual], velo_frame_to_frame through
 * the batch entries) then enqueues that promotion, the ingest and the index build BEHIND its own launches before its thread waits for them:
 * they run while the host reads the results and hands the pose over, and the next call finds the frame in place.  Until then the context is
 * one frame ahead -- any other job on it returns VELO_ERR_STATE.  A call that had to be repeated host-driven first gets its own pair back
 * (the old target's cloud is kept for that).  Results never change.  `next` itself is copied; the cloud and the ring table it names must
 * stay valid and unchanged until the call that brings the frame has returned (they are read during the announcing call's registration and
 * compared by the next one).  A scan that cannot be promoted or an announcement the loaders would refuse is not loaded ahead: the call that
 * brings it reports the error, as without the announcement. */
int velo_hint_next_frame(velo_ctx* ctx, const velo_scan_ref* next);

/* --- pose helpers (utility.h:67-96; note the reference's swapped names) ---------------- */
int velo_pose_vec_to_mat(const double x[6], double T[16]);  /* util::pose_mat2vec */
int velo_pose_mat_to_vec(const double T[16], double x[6]);  /* util::pose_vec2mat */
/* The pose hand-off of the drive loop (main.cpp:311-331,408) for n sequences at once, host arithmetic only: poses[i] (row-major 4x4,
 * in/out) <- poses[i] * dpose[i] (ceres_poses_mat[frame] = ceres_poses_mat[frame-1] * dpose), and x_next[i] <- the 6-vector of
 * poses_old[i]^-1 * poses_new[i] -- the constant-velocity guess the next frame's frameToFrame starts from.  x_next may be NULL. */
int velo_pose_handoff(int32_t n, double* poses /* n*16 */, const double* dpose /* n*16 */, double* x_next /* n*6 or NULL */);

/* --- multi-GPU: one process per GPU, RCCL over xGMI ---------------------------------- */
/* Query-sharded mode: every rank holds the whole target and a contiguous 1/world share of the query list;
 * each evaluation all-reduces the 28-double block (21 JtJ + 6 Jtr + cost) so all ranks take the same LM
 * decisions.  The 128-byte id comes from rank 0 and is distributed by the host program. */
int velo_comm_unique_id(char id[128]);
int velo_comm_init(velo_ctx* ctx, const char id[128], int32_t rank, int32_t world);
int velo_comm_destroy(velo_ctx* ctx);
/* The same mode without a collective library call per evaluation ("peer-mapped one-shot all-reduce"): every
 * rank owns a small slab in device memory; velo_comm_peer_export creates it and returns its 64-byte IPC handle
 * (hipIpcMemHandle_t); the host program gathers the handles of all ranks (rank order) and hands them to velo_comm_peer_attach,
 * which maps the peers' slabs.  Each LM step then writes its 28 doubles straight into every peer's slab and adds the world's
 * blocks in rank order inside the step kernel: deterministic, identical on all ranks, a few microseconds over xGMI instead of a
 * collective launch.  world <= 8.  Ranks may be processes on different GPUs of one node or -- for tests -- on the same GPU.
 * A peer that never arrives makes the wait time out (5 s): the call in flight (velo_frame_to_frame, velo_solve, velo_evaluate,
 * velo_associate in target-sharded mode) returns VELO_ERR_COMM, and the communicator must be exported and attached again on every rank
 * (the slabs' sequence numbers are out of step).  Every velo_comm_peer_export hands out a NEW, cleared slab (the previous one is
 * retired, not re-used: a slow peer's timed-out call may still be storing into it): every rank must have exported before any rank
 * attaches -- gathering the handles is that barrier -- and no barrier is needed between attach and the first call.
 * A chained call enqueues a predicted number of LM launches per solve, and over peers that number must be the same on every rank: the
 * ranks agree on it at the start of every chained call (the maximum over the ranks' own predictions, exchanged through the slabs),
 * so contexts with different call histories or VELO_CHAIN_MARGIN settings may share a communicator. */
int velo_comm_peer_export(velo_ctx* ctx, char handle[64]);
int velo_comm_peer_attach(velo_ctx* ctx, const char* handles /* world * 64 bytes, rank order */, int32_t rank, int32_t world);
/* Target-sharded mode over the same peers (instead of RCCL send/recv): the receive area for the per-query records of up to
 * max_queries queries (2 x (max_queries + 8 world) x 80 bytes), exported and attached like the slab, after velo_comm_peer_attach.
 * With it, velo_comm_set_target_sharded(ctx, 1) exchanges the records by direct stores into the owners' areas. */
int velo_comm_peer_export_records(velo_ctx* ctx, int32_t max_queries, char handle[64]);
int velo_comm_peer_attach_records(velo_ctx* ctx, const char* handles /* world * 64 bytes, rank order */, int32_t max_queries);
/* What is attached: kind 0 = nothing, 1 = RCCL communicator (world read back with ncclCommCount), 2 = peer slabs. */
int velo_comm_info(const velo_ctx* ctx, int32_t* kind, int32_t* rank, int32_t* world);
/* enable != 0: the communicator's ranks hold disjoint ring blocks of the target (velo_set_target_part) instead of
 * replicas; association then exchanges per-query top-2 records (all-to-all) before the query-sharded evaluation. */
int velo_comm_set_target_sharded(velo_ctx* ctx, int enable);
/* Restrict this context's queries to share `rank` of `world` WITHOUT a communicator (tests / replicas). */
int velo_set_query_shard(velo_ctx* ctx, int32_t rank, int32_t world);

/* Blocks until everything queued on the context's stream is done. */
int velo_synchronize(velo_ctx* ctx);

/* --- "next" row 3 of SURVEY.md 8(f): the producer of the 3-D keypoints rows R2-R4 consume ---------------- */
/* projectLidarToCamera (velo.h:329-374) for one camera, on the rings this context holds as source (of_target == 0) or target:
 * every point is shifted by cam_t (float, = cam_trans[cam]), projected c = (x/z, y/z) in float, kept when z > 0 and c lies in
 * [bounds[0], bounds[1]) x [bounds[2], bounds[3]) (= min_x, max_x, min_y, max_y of kitti.h:85-97, doubles), and pushed on the
 * ring's occlusion stack: entries behind it in x and farther in z are popped (velo.h:351-358), the point is dropped when the
 * stack top is right of it and nearer (velo.h:360-365).  Rings are independent; each is one sequential pass like the reference.
 * The surviving (`projection`, `scans_valid`) lists stay on the device for velo_depth_association. */
int velo_project_lidar(velo_ctx* ctx, int32_t of_target, const float cam_t[3], const double bounds[4], int32_t* n_valid_total);
/* copies the lists back: proj_xy [n][2], points_xyz [n][3] (the un-shifted points, velo.h:368), ring_offsets [n_rings + 1] */
int velo_get_projection(velo_ctx* ctx, float* proj_xy, float* points_xyz, int32_t capacity_points, int32_t* ring_offsets,
                        int32_t capacity_offsets, int32_t* n_rings);
/* featureDepthAssociation (velo.h:376-497) against the last velo_project_lidar: for every keypoint (canonical coordinates,
 * [n][2] floats) the first ring s whose bracketing segment and that of ring s-1 straddle the keypoint in y and are both
 * narrower than depth_assoc_thresh (kitti.h:28) gives a 3-D point by the reference's float bilinear interpolation.
 * has_depth[k] = -1 or the index into kp_with_depth (appended in keypoint order).  The reference's unqualified abs() on the
 * float widths (velo.h:416,419) is restated as fabs, like the outlier gate. */
int velo_depth_association(velo_ctx* ctx, const float* keypoints_xy, int32_t n_keypoints, double depth_assoc_thresh,
                           float* kp_with_depth_xyz, int32_t capacity_points, int32_t* has_depth, int32_t* n_with_depth);

/* --- "next" row 4: every landmark of a frame triangulated in one call (main.cpp:661-671 loops triangulatePoint over ids) ---
 * Landmark l owns obs[obs_offsets[l] .. obs_offsets[l+1]).  Residual blocks are added like velo.h:1049-1122: all 3-D
 * observations in the order given, then all 2-D observations in the order given (pass them cam-major, frame ascending --
 * the iteration order of the reference's per-camera std::map -- to reproduce its summation order).  Start value: the
 * current point when initial_guess[l] != 0, else (0, 0, 10) and, if there is a 3-D observation, a first solve on the first
 * 3-D block alone (velo.h:1080-1083).  The solver is the context's Ceres-default LM (velo_params), 3 unknowns.
 * camera_poses: [n_frames][6] (angle-axis, translation) as in ceres_poses_vec; cam_trans: [n_cams][3] floats.
 * points_xyz [n_landmarks][3] is read (initial guesses) and written (float, like pcl::PointXYZ); results may be NULL. */
int velo_triangulate_points(velo_ctx* ctx, const double* camera_poses, int32_t n_frames, const float* cam_trans, int32_t n_cams,
                            const velo_tri_obs* obs, const int32_t* obs_offsets, int32_t n_landmarks, float* points_xyz,
                            const uint8_t* initial_guess, velo_tri_result* results);

/* --- descriptor matching: matchFeatures (velo.h:499-560), the stage the reference runs on cv::cuda (USE_CUDA, velo.h:517-525) ----
 * One job = one (query set, train set) pair of 64-byte descriptors (FREAK, 512 bits), rows contiguous.  Per job, like
 * cv::BFMatcher(NORM_HAMMING).match and the filter after it (velo.h:527-549):
 *   train_idx[q] / distance[q]: the train row t with the smallest popcount(query[q] ^ train[t]), the LOWEST t on ties (the strict `<`
 *       of cv::BFMatcher); -1 / -1 when the job's train set is empty.
 *   min_dist: the smallest distance of the job (-1 when it has no match: an empty set; the reference's 1e9 then filters nothing).
 *   kept pairs (queryIdx, trainIdx), query order: distance <= max(1.5 * min_dist, match_thresh) (kitti.h:27: match_thresh = 29).
 * Outputs: train_idx / distance [sum n_query] (job-major, query order); min_dist / n_kept [n_jobs]; pairs [sum n_query][2], job j's
 * kept pairs starting at pair sum(n_kept[0..j-1]).  Every job of a call goes through ONE upload (a set named by several jobs --
 * the same pointer and row count -- travels once), one launch set and one copy back.  Train sets hold at most 2^22 rows.  The
 * context's registration state is untouched. */
typedef struct velo_desc_job {
    const uint8_t* query;   /* n_query x 64 bytes */
    int32_t n_query;
    const uint8_t* train;   /* n_train x 64 bytes */
    int32_t n_train;
} velo_desc_job;
int velo_match_descriptors(velo_ctx* ctx, const velo_desc_job* jobs, int32_t n_jobs, double match_thresh,
                           int32_t* train_idx, int32_t* distance, int32_t* min_dist, int32_t* n_kept, int32_t* pairs);

/* --- feature tracking: trackFeatures (velo.h:28-116), cv::calcOpticalFlowPyrLK four times per frame (main.cpp:220-245) -------------
 * Resident images: every context holds two image slots per camera, current and previous.  velo_set_images turns the current images
 * into the previous ones (a buffer rotation, no copy), uploads the new 8-bit grayscale frames (n_cams <= 8, all width x height,
 * rows `stride` bytes apart) in one copy and builds on the device each image's pyramid (cv::pyrDown, reflect-101) and the Scharr
 * derivatives of every level (calcSharrDeriv), which tracking reads once the image has become the previous one.  The levels kept are
 * those a 5-wide window would build, at most 7; every level is stored padded by 32 pixels (image reflect-101, derivatives zero).
 * The call is asynchronous (the next call on the context's stream waits for it).  The registration state is untouched. */
int velo_set_images(velo_ctx* ctx, const uint8_t* const* imgs, int32_t n_cams, int32_t width, int32_t height, int32_t stride);
/* Read-back of one padded level: kind 0 = image (uint8), 1 = dx, 2 = dy (int16); (height + 2 pad) x (width + 2 pad) values, row-major.
 * dims[4] receives the level's width, height, pad and the number of stored levels; out == NULL fills dims only. */
int velo_get_image_level(velo_ctx* ctx, int32_t cam, int32_t previous, int32_t level, int32_t kind, void* out, int64_t capacity_bytes,
                         int32_t* dims);
/* One job tracks n points (pixels, [n][2] floats) from the PREVIOUS image of prev_cam into the CURRENT image of cam, like
 * calcOpticalFlowPyrLK(img_prev, img, points1, points2, status, err, Size(window, window), max_level,
 * TermCriteria(COUNT | EPS, max_count, epsilon), 0, min_eig_threshold).  Outputs, job-major in job order: next_xy [sum n][2],
 * status [sum n] (calcOpticalFlowPyrLK's), kept [sum n] = the filters of velo.h:72-84: status set, util::dist2(p1, p2) (float
 * arithmetic, compared as double) <= flow_outlier, and p2 inside [0, width) x [0, height).  All jobs of a call share one upload,
 * one launch and one copy back.  The window sums are exact (int64) and rounded once to float. */
typedef struct velo_track_job {
    int32_t prev_cam;
    int32_t cam;
    const float* prev_xy;   /* n x 2 floats, pixels */
    int32_t n;
} velo_track_job;
typedef struct velo_lk_params {
    int32_t window;             /* odd, 5..31 (kitti.h:5: 21) */
    int32_t max_level;          /* 0..7 (kitti.h:6: 4) */
    int32_t max_count;          /* 0..100 (velo.h:64: 30) */
    int32_t reserved;
    double epsilon;             /* velo.h:65: 0.01 (compared squared, like OpenCV) */
    double min_eig_threshold;   /* OpenCV's default 1e-4 */
    double flow_outlier;        /* kitti.h:17: 20000 (pixels^2) */
} velo_lk_params;
int velo_track_features(velo_ctx* ctx, const velo_track_job* jobs, int32_t n_jobs, const velo_lk_params* p, float* next_xy,
                        uint8_t* status, uint8_t* kept);

/* --- corner detection: detectFeatures (velo.h:118-177), cv::GFTTDetector(corner_count, quality_level, min_distance) + the occupancy
 * filter against the frame's existing points, once per camera and frame (main.cpp:543-557) -----------------------------------------
 * Works on the CURRENT images of velo_set_images (an error if none was set): nothing is uploaded except the jobs' existing points.
 * One job detects on camera `cam`: cv::goodFeaturesToTrack(img, max_corners, quality_level, min_distance, noArray(), 3, false) --
 * the minimum-eigenvalue map (3 x 3 Sobel, 3 x 3 box sums, reflect-101), candidates above max * quality_level that are 3 x 3 local
 * maxima, in descending order of value (equal values: the higher row-major index first), greedy minimum-distance selection, at most
 * max_corners (<= 0: no cap) -- and flags every corner FRESH unless one of the job's existing points (pixels, [n][2] floats) lies at
 * util::dist2 (float arithmetic, compared as double) < (float)(min_distance^2) of it.  Existing points outside [0, width) x
 * [0, height) or non-finite take no part.  The box sums are exact integers.
 * Outputs, per job `capacity` entries apart: xy [n_jobs][capacity][2] (pixels, integral), response [n_jobs][capacity] (the map's
 * value), fresh [n_jobs][capacity], in selection order; counts [n_jobs][3] = corners, fresh corners, candidates.  A job whose corners
 * exceed `capacity` reports so in counts; the first `capacity` are written, entries past min(corners, capacity) are left untouched.
 * All jobs of a call share every launch and one synchronisation.  Registration state, image slots and pyramids are untouched. */
typedef struct velo_detect_job {
    int32_t cam;
    int32_t n_existing;
    const float* existing_xy;   /* n_existing x 2 floats, pixels */
} velo_detect_job;
typedef struct velo_gftt_params {
    int32_t max_corners;        /* kitti.h:7: 3000; <= 0: no cap */
    int32_t block_size;         /* 3 (GFTTDetector::create's default; the only supported value) */
    double quality_level;       /* kitti.h:18: 0.001; (0, 1] */
    double min_distance;        /* kitti.h:19: 12; [1, 64] */
} velo_gftt_params;
int velo_default_gftt_params(velo_gftt_params* p);
int velo_detect_features(velo_ctx* ctx, const velo_detect_job* jobs, int32_t n_jobs, const velo_gftt_params* p, int32_t capacity,
                         float* xy, float* response, uint8_t* fresh, int32_t* counts);
/* The minimum-eigenvalue map of the current image of `cam`: height x width floats, row-major (tests). */
int velo_get_corner_response(velo_ctx* ctx, int32_t cam, float* out, int64_t capacity_bytes);

/* --- the visual front end of several contexts in one call each ---------------------------------------------------------------------
 * A host thread that drives n sequences on one GPU calls these once per frame instead of the single-context entries n times.  The
 * contexts of a call must be distinct and on one device (at most 256); the FIRST one lends its stream, staging and scratch buffers.
 * A call runs after everything already enqueued on the stream of every context it names, and whatever is enqueued on any of them
 * later runs after the call's use of their buffers.  Every context ends in exactly the state, and every output byte is exactly the
 * one, that the single-context entries give when each context's share is handed to them in the same relative order; batch and single
 * calls may be mixed freely.  n_ctx == 1 IS the single-context entry.  Contexts may hold images of different sizes: the same launches
 * serve all of them (each unit's size travels in a device table), one launch set whatever n_ctx.  All arguments are checked before
 * any context is touched.
 *
 * velo_set_images_batch: imgs[i * n_cams + k] is camera k of context i; all images of ONE context share a size, sizes[3 i ..] =
 * {width, height, stride} of context i.  Per context what velo_set_images does, with one staged upload and one launch per pyramid
 * level for all of them.  Asynchronous like velo_set_images. */
int velo_set_images_batch(velo_ctx** ctxs, int32_t n_ctx, const uint8_t* const* imgs, int32_t n_cams, const int32_t* sizes /* n_ctx x 3 */);
/* velo_track_features / velo_detect_features over several contexts: job j runs on ctxs[job_ctx[j]] (its previous / current images).
 * Outputs are laid out exactly as by the single-context entries over the same job list (job-major, job order).  A context that no
 * job names is not touched and needs no images.  One upload, one launch (tracking) or one launch set (detection), one copy back, one
 * synchronisation.  A detection launch set carries at most 64 distinct cameras: a call that names more runs set after set, each with
 * its own upload, copy back and synchronisation, and if a later set fails (an allocation, a device error) the call returns the error
 * after the jobs of the earlier sets have already been written to the caller's arrays. */
int velo_track_features_batch(velo_ctx** ctxs, int32_t n_ctx, const int32_t* job_ctx, const velo_track_job* jobs, int32_t n_jobs,
                              const velo_lk_params* p, float* next_xy, uint8_t* status, uint8_t* kept);
int velo_detect_features_batch(velo_ctx** ctxs, int32_t n_ctx, const int32_t* job_ctx, const velo_detect_job* jobs, int32_t n_jobs,
                               const velo_gftt_params* p, int32_t capacity, float* xy, float* response, uint8_t* fresh, int32_t* counts);

/* --- the resident landmark store: the bookkeeping between the stages of a frame (main.cpp:376-386, main.cpp:614-679, velo.h:1132-1160) ---
 * Every context can hold one store: per landmark id keypoint_obs_count, keypoint_added and the landmark itself, every observation
 * (the entries of keypoint_obs2 / keypoint_obs3) in a log, and the Rodrigues constants of every frame's pose -- all on the device.
 * Per frame the caller hands over that frame's observations and pose only (one small upload per camera, one per pose) and the
 * triangulation is two launches.  How the cost of a frame compares with the stateless velo_triangulate_points as a sequence grows
 * has not been measured yet (tools/landmarks_bench.py is the measurement).  Both forms of the solve give the same bits.
 *
 * velo_landmarks_reset empties the store and fixes the cameras: cam_trans [n_cams][3] floats, n_cams 1..8.  log_capacity: entries
 * the observation log holds before it is first reallocated (0: the default, 65536; the ids of one landmark store cost 21 bytes of
 * device memory per id of the id space, so ids should be dense); the log, the id tables and the frame table all
 * grow geometrically.  A reallocation is the only time an observe / set_pose call waits for the device. */
int velo_landmarks_reset(velo_ctx* ctx, int32_t n_cams, const float* cam_trans, int32_t log_capacity);
/* ceres_poses_vec[frame] = pose6 (angle-axis, translation).  Frames may arrive in any order and may be set again; a triangulation
 * uses what was set last.  frame < 2^22. */
int velo_landmarks_set_pose(velo_ctx* ctx, int32_t frame, const double pose6[6]);
/* The loop body of main.cpp:622-645 for keypoints[cam][frame]: for entry i, obs_count[ids[i]]++ and the observation is kept as
 * keypoint_obs3[id][cam][frame] = kp_with_depth[has_depth[i]] when has_depth[i] != -1, else as keypoint_obs2[id][cam][frame] =
 * keypoints_xy[i] (canonical coordinates).  The id space grows as needed (main.cpp:614-621), ids < 2^26.  Refused with VELO_ERR_INVALID
 * before anything changes: a second call for the same (frame, cam), a negative id, an id twice in one call, a has_depth entry
 * outside [-1, n_with_depth).  n == 0 is a camera that saw nothing.  Asynchronous: the arrays are copied before the call returns. */
int velo_landmarks_observe(velo_ctx* ctx, int32_t frame, int32_t cam, const int32_t* ids, const float* keypoints_xy /* n x 2 */,
                           const int32_t* has_depth /* n */, const float* kp_with_depth_xyz /* n_with_depth x 3 */, int32_t n_with_depth,
                           int32_t n);
/* main.cpp:654-679 for `frame`: every id some camera observed in it, ascending (the std::set), with obs_count >= 3 is triangulated
 * from ALL its observations in the reference's block order (3-D observations camera-major and frame-ascending, then the 2-D ones
 * likewise), starting from its stored point when it was added before, else from (0, 0, 10) with the early solve on the first 3-D
 * block; the point is stored (float) and the id marked added.  Every frame that holds an observation needs its pose
 * (VELO_ERR_STATE otherwise).  Outputs in that id order: ids_out [capacity], points_out [capacity][3], results_out [capacity]
 * (each may be NULL); *n_out = the number triangulated -- when it exceeds `capacity` all of them are still solved and stored, the
 * first `capacity` are written.  One upload, one gather launch, one solve launch, one copy back, one synchronisation. */
int velo_landmarks_triangulate(velo_ctx* ctx, int32_t frame, int32_t* ids_out, float* points_out, velo_tri_result* results_out,
                               int32_t capacity, int32_t* n_out);
/* The same for frames[i] of ctxs[i], i < n_ctx, in ONE gather launch and ONE solve launch: a device table carries every context's
 * store, camera translations and velo_params (LM settings, loss), read per workgroup.  The rules of the front-end batch entries hold
 * (distinct contexts on one device, the first lends its stream and staging, batch and single calls mix freely, n_ctx == 1 IS the
 * single entry).  Outputs are context-major, `capacity` entries apart: ids_out [n_ctx][capacity], points_out [n_ctx][capacity][3],
 * results_out [n_ctx][capacity], n_out [n_ctx].  Every context's outputs and store are byte-identical to the single entry's. */
int velo_landmarks_triangulate_batch(velo_ctx** ctxs, int32_t n_ctx, const int32_t* frames, int32_t* ids_out, float* points_out,
                                     velo_tri_result* results_out, int32_t capacity, int32_t* n_out);
/* getLandmarksAtFrame (velo.h:1132-1160): for every id observed in `frame` that is added, p = pose_inv (x, y, z, 1) in double, each
 * row summed left to right, divided by p[3] and rounded to float; ascending id order (the std::map).  pose_inv16 is the row-major
 * INVERSE of the frame's pose, computed by the caller (the reference's Eigen inverse() is third-party arithmetic).
 * *n_out = the number of such landmarks; the first `capacity` are written. */
int velo_landmarks_at_frame(velo_ctx* ctx, int32_t frame, const double pose_inv16[16], int32_t* ids_out, float* xyz_out, int32_t capacity,
                            int32_t* n_out);
/* Read-back of landmarks->at(id), keypoint_added[id] and keypoint_obs_count[id] for n ids, from the device (outputs may be NULL);
 * an id beyond the store's id space reads as never seen. */
int velo_landmarks_get(velo_ctx* ctx, const int32_t* ids, int32_t n, float* xyz /* n x 3 */, uint8_t* added, int32_t* obs_count);
/* Host bookkeeping only, no device work: the distinct ids observed in `frame` and how many of them velo_landmarks_triangulate would
 * solve now (obs_count >= 3) -- the size its outputs need.  Either output may be NULL. */
int velo_landmarks_frame_count(velo_ctx* ctx, int32_t frame, int32_t* n_seen, int32_t* n_to_triangulate);
/* info[8] = ids in the id space, log entries, log capacity, log reallocations, frames in the frame table, cameras, (frame, cam)
 * pairs observed, 0. */
int velo_landmarks_info(velo_ctx* ctx, int32_t* info);

/* --- bundle adjustment of a window of frames over the landmark store (main.cpp:673-725, bundle2D / bundle3D costfunctions.h:222-286) ---
 * A joint refinement of poses and landmarks over the observations the store holds; nothing is uploaded but the frame list and the ids
 * the window's frames observed.
 *   frames    n_frames frame numbers, ascending and distinct, each with a pose set (VELO_ERR_STATE otherwise).  The first n_fixed
 *             (>= 1) are constants and fix the gauge; the other n_free = n_frames - n_fixed (1 .. 10) are unknowns, the 6 doubles of
 *             their ceres_poses_vec entry (angle-axis, centre).  n_frames x n_cams <= 64.
 *   landmarks take part if they are added, have at least 2 observations in window frames and at least one of them in a free frame;
 *             their point, widened from the stored float, is an unknown of 3 doubles.  Every other landmark keeps its bytes.
 *   residuals per landmark its window observations in the store's block order (3-D first, then 2-D, each camera-major and frame-
 *             ascending): bundle3D with weight = params->weight_3d and TrivialLoss; bundle2D with cam_trans[cam] and
 *             ScaledLoss(CauchyLoss(loss_thresh_3D2D), weight_3D2D) -- the losses velo_landmarks_triangulate uses, from velo_params.
 *   solver    Ceres' trust-region Levenberg-Marquardt over all unknowns with the settings of the context's
 *             velo_params; the linear step is the Schur complement on the landmark blocks.
 *   result    poses_out [n_frames][6]: the fixed frames as they were, the free frames refined.  The points are stored back as float and
 *             the store's frame table is refreshed as velo_landmarks_set_pose does it.  Parameters move on accepted steps only; two
 *             identical calls on identical state give identical bytes.
 * Refused before anything changes: VELO_ERR_INVALID for a NULL argument, frames that are not ascending, n_fixed < 1, n_free outside
 * 1 .. 10, n_frames x n_cams > 64, a weight that is not positive and finite; VELO_ERR_STATE without a store or for a frame without a
 * pose.  Not offered for several contexts in one call: their LM chains have different lengths. */
#define VELO_BA_MAX_FREE 10
#define VELO_BA_MAX_TRACE 50
#define VELO_BA_ACCEPTED 0      /* velo_ba_iteration.status */
#define VELO_BA_REJECTED 1
#define VELO_BA_INVALID 2       /* the linear solve failed or the model did not decrease: no evaluation */
#define VELO_BA_PARAMETER 3     /* ended by the parameter tolerance */
#define VELO_BA_FUNCTION 4      /* ended by the function tolerance */
#define VELO_BA_GRADIENT 5      /* accepted, then ended by the gradient tolerance */
typedef struct velo_ba_params {    /* 16 bytes */
    double weight_3d;          /* the `weight` of bundle3D; 1.0 */
    int32_t reserved[2];       /* 0 */
} velo_ba_params;
typedef struct velo_ba_iteration { /* 48 bytes */
    int32_t status;            /* VELO_BA_* */
    int32_t iteration;         /* from 1 */
    double cost;               /* at the iteration's start */
    double candidate_cost;     /* 0 for an invalid step */
    double radius;             /* at the iteration's start */
    double model_change;
    double step_norm;
} velo_ba_iteration;
typedef struct velo_ba_summary {   /* 48 + 50 x 48 bytes */
    int32_t termination;       /* VELO_CONVERGENCE / NO_CONVERGENCE / FAILURE */
    int32_t iterations;
    int32_t evaluations;
    int32_t n_landmarks;       /* that took part */
    int32_t n_blocks;
    int32_t n_residuals;
    int32_t n_trace;           /* records in trace: min(iterations, VELO_BA_MAX_TRACE) */
    int32_t reserved;
    double initial_cost;
    double final_cost;
    velo_ba_iteration trace[VELO_BA_MAX_TRACE];
} velo_ba_summary;
int velo_default_ba_params(velo_ba_params* params);
/* params may be NULL (the defaults); poses_out and summary may be NULL. */
int velo_landmarks_adjust(velo_ctx* ctx, const int32_t* frames, int32_t n_frames, int32_t n_fixed, const velo_ba_params* params,
                          double* poses_out /* n_frames x 6 */, velo_ba_summary* summary);
/* Diagnostics: the problem velo_landmarks_adjust would solve, evaluated at the stored state; nothing changes.  cost, the poses' part of
 * J^T r (gradient [6 n_free]) and the poses' diagonal blocks of J^T J (JtJ_pose [n_free][36], row-major), robustified, unscaled. */
int velo_landmarks_adjust_system(velo_ctx* ctx, const int32_t* frames, int32_t n_frames, int32_t n_fixed, const velo_ba_params* params,
                                 double* cost, double* gradient, double* JtJ_pose);

/* --- the pose graph of a drive and its batch optimisation (main.cpp:190-204, main.cpp:516-536, main.cpp:728-745) ---
 * Every context can hold one pose graph: one node per frame and every accepted registration as an edge, on the device.  What
 * velo_graph_optimize returns is what velo_landmarks_set_pose and velo_map_set_pose take: the corrected poses of a loop closure.
 *   nodes     the 6 doubles of ceres_poses_vec[frame] (angle-axis, translation): the world pose of camera 0.  The reference's nodes of
 *             the other cameras hang on it by noiseless6 extrinsic factors (main.cpp:196-203, 526-534): rigid copies, not modelled.
 *   edges     (from, to, z, info) states pose_to = pose_from . Z, Z = pose_mat2vec(z): what frameToFrame returns (main.cpp:408,
 *             518-524).  The residual is sqrt(info) x pose_vec2mat(Z^-1 . T_from^-1 . T_to), the angle-axis of the rotation and then the
 *             translation -- the form of main.cpp:416-424; info is the s of Information(s . eye(6)) (noisy6: 1, noiseless6: 1000); the
 *             loss is trivial.  Duplicate edges add up.
 *   gauge     fixed nodes are constants (the reference's prior of weight 1000 on node 0 becomes "node 0 is fixed"); at least one.  An
 *             edge between two fixed nodes adds its constant cost only.  A free node no edge touches keeps its bytes.
 *   solver    Ceres' trust-region Levenberg-Marquardt over every node that has a pose and is not fixed, with the
 *             settings of the context's velo_params and Jacobi scaling; the linear step is a block-Jacobi preconditioned conjugate
 *             gradient on the damped normal equations, stopped when sqrt(r.M^-1 r) has fallen to cg_tolerance of its start or after
 *             cg_max_iterations.  iSAM's own parametrisation (Euler angles), its Gauss-Newton / dog-leg and its incremental smoothing are
 *             not reproduced.  Parameters move on accepted steps only; two identical calls on identical state give
 *             identical bytes.
 *   envelope  params->reserved[0] selects the linear solver of a call.  VELO_GRAPH_SOLVER_CG (0, the default) is the CG above.
 *             VELO_GRAPH_SOLVER_ENVELOPE (1) factors the same damped, Jacobi-scaled normal equations exactly: a block-skyline (envelope)
 *             Cholesky in the reverse Cuthill-McKee order of the free nodes that velo_graph_order states, one workgroup per LM
 *             iteration, then a forward and a back substitution.  It needs no tolerance, cap or preconditioner: cg_tolerance and
 *             cg_max_iterations are validated and otherwise ignored, and every trace record has cg_iterations = 0, cg_residual = 0.  A
 *             loop closure costs band width, not fill, so a whole drive converges where the CG runs into its cap.
 *             params->reserved[1] caps its work, in 6 x 6 block products per factorisation: work = sum_i w_i (w_i + 1) / 2 with
 *             w_i = i - first(i) in that order; 0 is the default, VELO_GRAPH_DEFAULT_MAX_WORK.  A graph whose order exceeds the cap is
 *             refused with VELO_ERR_INVALID before a pose moves (the message states the work, the cap and the widest row): the caller can
 *             fall back to the CG.  Any other reserved[0] and a negative reserved[1] are refused with VELO_ERR_INVALID.
 *   weighted  velo_graph_add_edges_weighted gives an edge a 6 x 6 information W and, optionally, a robust loss.  For edge e let r be the
 *             UNWEIGHTED 6-vector pose_vec(Z^-1 . T_from^-1 . T_to) (rotation, then translation) and A, B its Jacobians with respect to
 *             the two nodes.  s = r^T W r, W symmetric positive definite in the residual's order.  The edge's cost term is rho(s) / 2:
 *             rho(s) = s for the trivial loss (loss_scale 0), rho(s) = b ln(1 + s / b), b = a^2, for Cauchy(a) (loss_scale a > 0;
 *             ceres::CauchyLoss(a)).  The normal-equation blocks are rho'(s) . A^T W A, rho'(s) . B^T W B, rho'(s) . A^T W B and the
 *             gradients rho'(s) . A^T W r, rho'(s) . B^T W r: Ceres' corrector in its rho'' <= 0 branch (residual and Jacobian scaled
 *             by sqrt(rho'), alpha = 0) -- Cauchy's rho'' is negative everywhere, so this is Ceres' behaviour, not an approximation.
 *             W is stored as its Cholesky factor, W = L L^T, and s is formed as |L^T r|^2.  The trust-region controller, both linear
 *             solvers, velo_graph_system, the summary's costs and the trace see the weighted, robustified problem.  Once a store holds
 *             a weighted edge, a scalar edge is info . I with the trivial loss there, whether it was added before or after; the two
 *             entries mix freely and edge order is addition order.  A store that never saw a weighted edge runs the scalar kernel
 *             and gives the bytes it always gave; velo_graph_reset returns a store to that state.  The reference's noisy6 (isotropic,
 *             trivial loss) stays the default; matrix information and Cauchy are this library's additions.
 * velo_graph_reset creates or empties the store; edge_capacity: edges the device arrays hold before they are first reallocated (0: the
 * default, 4096); they grow by doubling.  Frames < 2^22.  Refused before anything changes: VELO_ERR_INVALID for a NULL argument, a frame
 * out of range, from == to, a non-finite pose or z, an info that is not positive and finite, fixed frames that are not ascending and
 * distinct, n_fixed < 1; VELO_ERR_STATE without a store, for a fixed frame or an edge's end without a pose. */
#define VELO_GRAPH_MAX_TRACE 50
#define VELO_GRAPH_SOLVER_CG 0                   /* reserved[0]: block-Jacobi preconditioned CG (the default) */
#define VELO_GRAPH_SOLVER_ENVELOPE 1             /* reserved[0]: envelope Cholesky in reverse Cuthill-McKee order */
#define VELO_GRAPH_DEFAULT_MAX_WORK (1 << 24)    /* reserved[1] == 0: block products per factorisation the envelope solver accepts */
typedef struct velo_graph_params {     /* 32 bytes */
    double cg_tolerance;       /* relative, on sqrt(r.M^-1 r); 1e-10: the inexact step then takes the LM decisions of a direct solve */
    int32_t cg_max_iterations; /* per LM iteration; 2000 */
    int32_t reserved[5];       /* [0]: VELO_GRAPH_SOLVER_*; [1]: the envelope solver's work cap (0: the default); [2..4]: 0 */
} velo_graph_params;
typedef struct velo_graph_iteration {  /* 64 bytes: velo_ba_iteration, then the linear solve */
    int32_t status;            /* VELO_BA_* */
    int32_t iteration;         /* from 1 */
    double cost;               /* at the iteration's start */
    double candidate_cost;     /* 0 for an invalid step */
    double radius;             /* at the iteration's start */
    double model_change;
    double step_norm;
    int32_t cg_iterations;
    int32_t reserved;
    double cg_residual;        /* sqrt(r.M^-1 r) over its start when CG stopped */
} velo_graph_iteration;
typedef struct velo_graph_summary {    /* 48 + 50 x 64 bytes */
    int32_t termination;       /* VELO_CONVERGENCE / NO_CONVERGENCE / FAILURE */
    int32_t iterations;
    int32_t evaluations;
    int32_t n_nodes;           /* that have a pose */
    int32_t n_free;
    int32_t n_edges;
    int32_t n_trace;           /* records in trace: min(iterations, VELO_GRAPH_MAX_TRACE) */
    int32_t reserved;
    double initial_cost;
    double final_cost;
    velo_graph_iteration trace[VELO_GRAPH_MAX_TRACE];
} velo_graph_summary;
int velo_default_graph_params(velo_graph_params* params);
int velo_graph_reset(velo_ctx* ctx, int32_t edge_capacity);
/* one node, or the run first .. first + n - 1 (poses [n][6]); a node that has a pose is overwritten */
int velo_graph_set_pose(velo_ctx* ctx, int32_t frame, const double pose6[6]);
int velo_graph_set_poses(velo_ctx* ctx, int32_t first, int32_t n, const double* poses);
/* appends n edges: from [n], to [n], z [n][6], info [n] */
int velo_graph_add_edges(velo_ctx* ctx, int32_t n, const int32_t* from, const int32_t* to, const double* z, const double* info);
/* n edges with a full information matrix and, optionally, a robust loss.
 * info21: [n][21], the upper triangle of W row by row ((0,0),(0,1)..(0,5),(1,1)..).
 * loss_scale: [n] or NULL (all trivial): 0 = trivial, a > 0 = Cauchy(a) on s = r^T W r.
 * Refuses what velo_graph_add_edges refuses, and with VELO_ERR_INVALID a NULL info21, a non-finite entry, a W whose Cholesky
 * factorisation in double meets a pivot that is not positive and finite (the message names the edge's index in the call), a loss_scale
 * that is negative or not finite.  A refused call changes nothing. */
int velo_graph_add_edges_weighted(velo_ctx* ctx, int32_t n, const int32_t* from, const int32_t* to, const double* z, const double* info21,
                                  const double* loss_scale);
/* Per edge, in the order the edges were added (both entries count), at the STORED poses: chi2[i] = s, weight[i] = rho'(s) (1 for a
 * trivial edge; a scalar-only store answers info . |r|^2 and 1, and stays scalar-only).  Nothing changes.  Either output may be NULL.
 * VELO_ERR_STATE without a store or for an end without a pose, VELO_ERR_INVALID for a range outside [0, edges]. */
int velo_graph_edge_stats(velo_ctx* ctx, int32_t first, int32_t n, double* chi2, double* weight);
/* A registration's information as an edge's: a pure host function, no context, no GPU.  z: the registration's result; JtJ36: its 6 x 6
 * at that result, as velo_evaluate returns it.  Writes W as info21: W = Bz^-T H Bz^-1, Bz = blockdiag(Rz^T J_l(w_z), Rz^T), the
 * Jacobian of the edge residual with respect to the pose 6-vector at x = z; H is symmetrised as (H + H^T) / 2 first.  VELO_ERR_INVALID
 * for a NULL or non-finite input.  Definiteness is not tested here: velo_graph_add_edges_weighted does that, and a caller may add
 * eps . I in between. */
int velo_graph_edge_information(const double z[6], const double JtJ36[36], double info21[21]);
/* fixed: n_fixed frames, ascending and distinct, each with a pose.  params may be NULL (the defaults), summary may be NULL. */
int velo_graph_optimize(velo_ctx* ctx, const int32_t* fixed, int32_t n_fixed, const velo_graph_params* params, velo_graph_summary* summary);
/* poses of first .. first + n - 1 to out [n][6]; VELO_ERR_STATE when one of them has no pose */
int velo_graph_get_poses(velo_ctx* ctx, int32_t first, int32_t n, double* out);
/* info[8] = nodes with a pose, edges, edge capacity, edge reallocations, frames of the node table, optimisations run, and of the
 * context's last envelope solve the widest row and the envelope's block count (both 0 until there has been one) */
int velo_graph_info(velo_ctx* ctx, int32_t* info);
/* The order the envelope solver factors in; a pure host function: no context, no GPU.  Nodes are 0 .. n_nodes - 1 (for
 * velo_graph_optimize: the free nodes in ascending frame order), edges (a[e], b[e]) join two of them (edges that touch a fixed node
 * are the caller's to drop); duplicates and both directions are merged.  perm[k] is the node at position k, first[k] the smallest
 * position among k and its neighbours, stats[4] = the widest row max w_k (w_k = k - first[k]), the envelope blocks sum (w_k + 1), the
 * work sum w_k (w_k + 1) / 2, the number of components.  The rule, to the letter:
 *   degree      the number of distinct neighbours;
 *   components  in ascending order of their smallest node;
 *   start node  George-Liu's pseudo-peripheral node: begin at the component's node of least degree (lowest index on a tie) and
 *               build its breadth-first level structure; take from the last level the node of least degree (lowest index on a tie)
 *               and build its level structure; if that has strictly more levels, go on from that node, otherwise keep the node at hand;
 *   Cuthill-McKee  from the start node; a dequeued node's unvisited neighbours are appended in ascending (degree, index);
 *   result      the sequence of all components, reversed as a whole.
 * A node without a neighbour is a component of its own and a row of width 0.  VELO_ERR_INVALID: a NULL argument (a and b may be NULL
 * when n_edges is 0), a negative count, an end out of range, a[e] == b[e]. */
int velo_graph_order(int32_t n_nodes, int32_t n_edges, const int32_t* a, const int32_t* b, int32_t* perm, int32_t* first, int64_t* stats);
/* The order of a graph that has GROWN since an order of it was kept (velo_graph_retain); a pure host function: no context, no GPU.
 * perm_old [n_old] is the kept order of the nodes 0 .. n_old - 1; the nodes n_old .. n_nodes - 1 are new; a, b are ALL edges, of which
 * those from first_new_edge on are new (an edge before it joins two old nodes).  Writes perm [n_nodes], first [n_nodes] and stats[8].
 * The rule, to the letter:
 *   extended order   perm_old, then the new nodes in ascending number;
 *   first dirty row  p = the smallest position, in the extended order, among the ends of the new edges and the new nodes; p = n_nodes
 *                    when there is nothing new.  A Cholesky factor in the extended order keeps every row before p;
 *   rows before p    keep their `first`: no new edge touches them.  The function checks it (VELO_ERR_STATE if not: cannot happen);
 *   rows >= p        `first` as velo_graph_order defines it, over all edges;
 *   fresh order      velo_graph_order's order of the whole graph, ORIENTED: it is reversed as a whole when both hold: the reversal moves
 *                    the highest-numbered node from the first half of the positions to the second (2 pos < n_nodes before and
 *                    2 (n_nodes - 1 - pos) >= n_nodes after), and the reversed order's work is <= VELO_GRAPH_RETAIN_REBUILD_RATIO times the
 *                    unreversed one's.  (A chain's newest frame must sit near the end of the order, or every later append dirties row 0);
 *   rebuild          the extended order is the result iff its work sum w (w + 1) / 2 is <= max_work AND <=
 *                    VELO_GRAPH_RETAIN_REBUILD_RATIO times the fresh order's; otherwise the result is the fresh order and p = 0.  A fresh
 *                    order over max_work is still returned: the caller compares stats[2];
 *   stats            [0] widest row, [1] blocks, [2] work, [3] components, all of the result; [4] p; [5] 1 if the result is the fresh
 *                    order (a rebuild); [6] 1 if it is the fresh order reversed; [7] the fresh order's work.
 * With n_old == 0 the extended order is 0, 1, .. n_nodes - 1: what velo_graph_retain starts from without a caller's order.
 * VELO_GRAPH_RETAIN_REBUILD_RATIO is a policy constant: how much factorisation work an append may cost over a fresh order before the
 * order is built anew.  It is NOT measured or tuned; profiles/ records what it costs where it was tried.
 * VELO_ERR_INVALID: a NULL argument (perm_old may be NULL when n_old is 0, a and b when n_edges is 0), a negative count or max_work,
 * n_nodes < n_old, first_new_edge outside 0 .. n_edges, a perm_old that is not a permutation of 0 .. n_old - 1, an end out of range,
 * a[e] == b[e], an edge before first_new_edge that ends at a new node. */
#define VELO_GRAPH_RETAIN_REBUILD_RATIO 2
int velo_graph_order_extend(int32_t n_old, const int32_t* perm_old, int32_t n_nodes, int32_t n_edges, const int32_t* a, const int32_t* b,
                            int32_t first_new_edge, int64_t max_work, int32_t* perm, int32_t* first, int64_t* stats);
/* Diagnostics: the problem velo_graph_optimize would solve, evaluated at the stored state; nothing changes.  The free nodes are the
 * nodes with a pose that are not fixed, ascending: cost, J^T r (gradient [n_free][6]) and the diagonal blocks of J^T J (diag_blocks
 * [n_free][36], row-major), unscaled.  Each output may be NULL. */
int velo_graph_system(velo_ctx* ctx, const int32_t* fixed, int32_t n_fixed, double* cost, double* gradient, double* diag_blocks);
/* Marginal and joint covariances of the poses (what iSAM offers as slam.covariances()), evaluated at the stored state; nothing in the
 * store changes.  The free nodes are those of velo_graph_optimize with the same `fixed`.  H = J^T J is the UNDAMPED normal matrix of
 * the problem the solvers see: the Jacobian whitened by sqrt(info) or by the Cholesky factor of W, corrected by the robust loss where
 * an edge has one.  Sigma = H^-1, in the coordinates the solver steps in (the 6 doubles of a node): Ceres' Covariance convention for
 * cost = sum |r|^2 / 2.  Pair p returns Cov(frame_a[p], frame_b[p]) as cov36[p], row-major 6 x 6: the marginal for a == b, the cross
 * block Sigma_ab (not its transpose) otherwise; a pair that names a fixed frame returns 36 zeros (a constant has no uncertainty).
 * (a, b) and (b, a) are transposes of one another to the bit, a marginal is symmetric to the bit, and two identical calls give
 * identical bytes.
 *   method    the Jacobi-scaled H is factored by the envelope Cholesky in the order of velo_graph_order; the entries of its inverse
 *             inside the envelope follow from the factor by the Takahashi recursion (one workgroup, the factorisation's block-product
 *             count): every marginal and the pair of every edge between free nodes lie there.  A pair outside the envelope costs a
 *             column solve of its own (forward and back substitution with 6 right-hand sides) over a work vector of n_free x 36
 *             doubles; pairs in different components of the free graph return an exact zero block.
 *   params    only reserved[1], the envelope's work cap, is read (NULL, or 0 there: VELO_GRAPH_DEFAULT_MAX_WORK); the other members
 *             are validated as velo_graph_optimize validates them.
 * Refused before anything is written to cov36: what velo_graph_optimize refuses; VELO_ERR_INVALID for n_pairs < 0, a NULL array with
 * n_pairs > 0, a frame out of range, an order whose work exceeds the cap (the envelope solver's message), pairs outside the envelope
 * whose work vectors exceed VELO_GRAPH_MAX_COLUMN_DOUBLES in all, and an H that is not positive definite -- the message names the frame
 * of the failing pivot; a free node without edges is the case; VELO_ERR_STATE for a frame without a pose. */
#define VELO_GRAPH_MAX_COLUMN_DOUBLES (1 << 27)  /* work vectors of one call's pairs outside the envelope: pairs x n_free x 36 doubles (1 GiB) */
int velo_graph_covariance(velo_ctx* ctx, const int32_t* fixed, int32_t n_fixed, const velo_graph_params* params,
                          int32_t n_pairs, const int32_t* frame_a, const int32_t* frame_b, double* cov36 /* [n_pairs][36] row-major */);
/* The covariance of a relative pose in an edge's tangent space, and the test of a proposed edge BEFORE it enters the graph (the
 * reference's agreement check, main.cpp:415-437, has no statistics behind it).  Evaluated at the stored state; nothing in the store
 * changes.  Free nodes, H, params (only reserved[1] is read) and the factorisation are velo_graph_covariance's.  For pair p, with
 * a = from[p], b = to[p] and the stored poses:
 *   rel6    pose_vec(T_a^-1 T_b);
 *   z       the measurement Z_p; NULL: every pair takes its own rel6, formed on the device;
 *   r6      the unweighted edge residual pose_vec(Z_p^-1 T_a^-1 T_b) -- evaluated, not assumed zero;
 *   cov36   S = Sigma_rel + W^-1, row-major, symmetric to the bit.  Sigma_rel = A S_aa A^T + A S_ab B^T + B S_ba A^T + B S_bb B^T with A, B
 *           the Jacobians of r in the 6 doubles of a and b and the S blocks exactly what velo_graph_covariance returns (zero for a fixed
 *           frame): to first order the covariance of r, which -- unlike the marginals -- does not depend on which frame is fixed.  W is
 *           info21[p] (the upper triangle row by row, as velo_graph_add_edges_weighted takes it); NULL: S = Sigma_rel;
 *   chi2    r^T S^-1 r through the Cholesky factor of S in double; -1.0 where a pivot of S is not positive and finite (both ends fixed
 *           and no info21 is the case).
 * Every output may be NULL.  What a caller should know:
 *   - the result belongs to the estimate H describes: Sigma is the covariance AT THE OPTIMUM, so optimise first.  At a dead-reckoned
 *     start a true closing edge gates at chi2 in the hundreds;
 *   - chi2 means something only if the edges' informations are inverse covariances (velo_graph_edge_information), not weights;
 *   - chi2 is compared with a quantile of the chi-square distribution with 6 degrees of freedom (16.8 at 99 %, 22.5 at 99.9 %); the
 *     threshold and what to do with the edge are the caller's.
 *   cost    blocks inside the envelope come from the selected inverse.  The pairs outside it are grouped by their `to` frame and ONE
 *           full block column of the inverse is solved per distinct such frame (n_free x 36 doubles of work vector each, under
 *           VELO_GRAPH_MAX_COLUMN_DOUBLES in all): 32 candidates against one query frame cost one column, not 32.
 * Refused before anything is written: what velo_graph_covariance refuses (and, as there, a call with n == 0 returns VELO_OK after the
 * argument checks alone: no order is formed and nothing is factored, so neither the work cap nor H is tested); VELO_ERR_INVALID for
 * n < 0, a NULL from or to with n > 0, a
 * frame out of range, from == to, a z that is not finite, an info21 that velo_graph_add_edges_weighted would refuse (the message names
 * the pair); VELO_ERR_STATE for a frame without a pose. */
int velo_graph_edge_gate(velo_ctx* ctx, const int32_t* fixed, int32_t n_fixed, const velo_graph_params* params,
                         int32_t n, const int32_t* from, const int32_t* to, const double* z /* [n][6] | NULL */, const double* info21 /* [n][21] | NULL */,
                         double* rel6 /* [n][6] */, double* r6 /* [n][6] */, double* cov36 /* [n][36] */, double* chi2 /* [n] */);
/* Loop-closure candidates for one query frame, proposed from the graph (the reference tries fixed offsets and divides the vertical
 * component by 20 by hand because height drifts, main.cpp:328-345; the graph knows how uncertain each relative position is).  Considers
 * every frame i that has a pose with |i - query| >= min_gap:
 *   dist    |t(T_i^-1 T_query)| at the stored poses;
 *   sigma   sqrt(trace(Sigma_rel(i, query)[3:, 3:])) in the tangent at the stored relative pose: the total standard deviation of the
 *           relative position (the trace does not depend on the frame it is written in);
 * and selects i when dist <= radius + k_sigma . sigma.  The selected frames are returned in ascending order: the first `capacity` are
 * written to frames_out, dist_out, sigma_out (each [capacity], each may be NULL), *n_found is the total -- ask again with more room when
 * it exceeds capacity.  What velo_match_frames then screens.  Work: one factorisation, one selected inverse, ONE full block column
 * for the query (none when it is fixed), a thread per frame and an ordered compaction.  Frames in another component of the free graph
 * have a zero cross-covariance, exactly.  k_sigma == 0 is the reference's test without its /20: no factorisation runs, sigma is
 * written as 0, and a graph whose H is singular is served.  As for velo_graph_edge_gate, sigma belongs to the optimum.
 * Refused before anything is written: what velo_graph_covariance refuses (with k_sigma == 0: what its argument checks refuse);
 * VELO_ERR_INVALID for a query out of range, min_gap < 1, a radius or k_sigma that is negative or not finite, capacity < 0, a NULL
 * n_found; VELO_ERR_STATE for a query without a pose. */
int velo_graph_loop_candidates(velo_ctx* ctx, const int32_t* fixed, int32_t n_fixed, const velo_graph_params* params,
                               int32_t query, int32_t min_gap /* >= 1 */, double radius /* >= 0 */, double k_sigma /* >= 0 */,
                               int32_t capacity, int32_t* frames_out, double* dist_out, double* sigma_out, int32_t* n_found);
/* Retains the factorisation the three entries above build -- velo_graph_covariance's problem for the stored state and this `fixed` set:
 * the same free nodes, the same undamped H, the same Jacobi scales, the work cap of params->reserved[1] -- so that they stop building it
 * per call.  Kept, in buffers of its own: the order's ints, the skyline of L, the scales, the poses; on first need the skyline of Z (the
 * selected inverse, at most once per generation) and the LAST full block column solved, with its position: a candidates call for frame q
 * followed by gates whose `to` is q solves one column.  A context retains one state; retaining again replaces it.
 *   perm     the order to factor in: a permutation of the free nodes' indices, n_perm == n_free; with velo_graph_order's order the
 *            factorisation, and so every answer, is to the bit the one an un-retained call computes.  NULL: velo_graph_order_extend's
 *            rule with n_old == 0 (frame order, unless that costs more than VELO_GRAPH_RETAIN_REBUILD_RATIO times the fresh order);
 *   queries  velo_graph_covariance, velo_graph_edge_gate and velo_graph_loop_candidates with k_sigma > 0 use the state when their
 *            `fixed` equals the retained one and their cap is not below the retained one; otherwise they run as without it and leave it
 *            alone.  On a current state they build no order, fill and factor nothing;
 *   append   frames posed for the first time whose numbers lie above every retained free frame, and new edges, leave the state BEHIND.
 *            The next such query, or the next velo_graph_retain with perm == NULL, extends it: the order of velo_graph_order_extend, the
 *            system linearised and assembled again, the rows from the first dirty row on filled and factored -- the rows before keep
 *            their bits, and the rows after get the bits of a full factorisation in that order.  Z and the kept column go stale.  Where
 *            the rule says rebuild, everything is rebuilt in the fresh order.  An extension that fails (the cap; a pivot that is not
 *            positive, as of a new frame that has no edge yet) leaves the state behind at its last good generation -- the rows it
 *            touched are filled again by the next extension -- and the call is answered, or refused, as without a state;
 *            an extension over the cap fails again, after forming the system, on every such query until velo_graph_release or a
 *            velo_graph_retain under a larger cap.  The extension runs BEFORE the query's own later checks: a query that is then
 *            refused (its column work vectors over VELO_GRAPH_MAX_COLUMN_DOUBLES) has written nothing to its outputs and nothing to
 *            the store, but may have moved the retained state on by a generation, counters included;
 *   dropped  by velo_graph_set_pose[s] on a frame that has a pose, a newly posed frame numbered below a retained free frame,
 *            velo_graph_optimize once it runs (whatever its outcome: retain again after a solve), velo_graph_reset, and the store's
 *            promotion to weighted edges.  The queries then run as without a state.
 * Refused: what velo_graph_covariance refuses; VELO_ERR_INVALID for a perm that is not a permutation, work over the cap (both leave a
 * state retained before as it was) and an H that is not positive definite (the message names the frame; nothing is retained then).
 * velo_graph_release forgets the state and frees its buffers; without one it returns VELO_OK.  velo_graph_retained reports:
 *   info[0] state: 0 none, 1 current, 2 behind     [1] free nodes in the retained order   [2] widest row   [3] blocks   [4] work
 *   counters since velo_graph_reset or velo_graph_release:  [5] full builds   [6] extensions   [7] of them rebuilds forced by the order's
 *   rule   [8] selected-inverse runs   [9] full columns solved   [10] queries served from the state
 *   [11] the first dirty row of the last extension   [12] the rows it refactored   [13..15] 0
 * and the first min(capacity, info[1]) entries of the order in perm_out (NULL with capacity 0).  velo_graph_info is unchanged. */
int velo_graph_retain(velo_ctx* ctx, const int32_t* fixed, int32_t n_fixed, const velo_graph_params* params,
                      const int32_t* perm /* [n_perm] | NULL */, int32_t n_perm);
int velo_graph_release(velo_ctx* ctx);
int velo_graph_retained(velo_ctx* ctx, int64_t info[16], int32_t* perm_out, int32_t capacity);

/* --- resident keypoint frames and the visual matches assembled from them (velo.h:562-590, velo.h:627-654, main.cpp:366-405) ---
 * Every context can hold one frame store: for every (frame, camera) put so far keypoints[cam][frame], keypoint_ids[cam][frame],
 * has_depth[cam][frame] and keypoints_with_depth[cam][frame], in one device arena; the host keeps a directory (frame, cam) ->
 * offset, n, n_with_depth, largest id, and the list of free blocks (first-fit, blocks are neither split nor merged: made for a
 * sliding window of frames of similar size) -- no copy of the arrays.  velo_build_matches joins two such frames by id (matchUsingId), substitutes the
 * landmarks of the context's landmark store (velo.h:634-644), gathers every match's operands (velo.h:645-654) and leaves the
 * records in the context's visual set, as velo_set_visual would: the records never exist on the host, and a landmark triangulated
 * on the device is not read back only to be sent down again.  What the host work it replaces costs has not been measured yet
 * (tools/visual_assembly_bench.py is the measurement).
 *
 * velo_frames_reset empties the store and fixes the cameras: cam_trans [n_cams][3] floats, n_cams 1..8 (as the landmark store).
 * arena_capacity: bytes the arena holds before it is first reallocated (0: the default, 1 MiB); it grows geometrically, and a
 * reallocation is the only time velo_frames_put waits for the device. */
int velo_frames_reset(velo_ctx* ctx, int32_t n_cams, const float* cam_trans, int32_t arena_capacity);
/* keypoints[cam][frame] with their ids, has_depth (-1 or an index into kp_with_depth_xyz) and the cloud: the argument list of
 * velo_landmarks_observe, so a caller hands both the same arrays.  A second call for the same (frame, cam) REPLACES the entry (the
 * reference mutates a frame's arrays until the frame ends), in place when it fits.  n == 0 is valid and counts as put.  An id may
 * occur more than once (matchUsingId has a rule for it, below).  Refused with VELO_ERR_INVALID before anything changes: a negative
 * id, an id >= 2^26, a has_depth entry outside [-1, n_with_depth).  frame < 2^22.  Asynchronous: the arrays are copied into pinned
 * memory before the call returns, one upload, no synchronisation and no device allocation in the steady state. */
int velo_frames_put(velo_ctx* ctx, int32_t frame, int32_t cam, const int32_t* ids, const float* keypoints_xy /* n x 2 */,
                    const int32_t* has_depth /* n */, const float* kp_with_depth_xyz /* n_with_depth x 3 */, int32_t n_with_depth,
                    int32_t n);
/* Frees every camera's entry of `frame` for reuse (a frame that is not held: nothing happens). */
int velo_frames_drop(velo_ctx* ctx, int32_t frame);
/* Host bookkeeping only: n_per_cam [n_cams] (may be NULL) = the keypoints of every camera's entry of `frame` as put (-1: never put
 * or dropped), *n_total (may be NULL) their sum -- no registration against `frame` as frame2 has more matches, which sizes pairs_out. */
int velo_frames_count(velo_ctx* ctx, int32_t frame, int32_t* n_per_cam, int32_t* n_total);
/* info[8] = frames held, (frame, cam) entries, arena bytes, arena reallocations, arena bytes handed out so far, cameras, ids per
 * camera the slot table holds, free blocks.  The two byte counts saturate at 2^31 - 1. */
int velo_frames_info(velo_ctx* ctx, int32_t* info);
/* The visual set of frameToFrame(frame1, frame2) (frame1 the current frame, frame2 the previous one).  Per camera, in camera order:
 * matchUsingId -- for ind2 ascending over frame2's ids, when the id occurs in frame1, the match (ind1, ind2) with ind1 the LAST
 * index of frame1 that holds it (the id2ind[id] = ind overwrite of velo.h:571-574); an id twice in frame2 gives two matches.  Per
 * match the velo_match record of velo.h:630-654: d1 / p3_1 from frame1's has_depth; p3_2 = the landmark of that id moved by
 * pose2_inv16 (the arithmetic and the bits of velo_landmarks_at_frame) and d2 = 1 when pose2_inv16 is given, the context has a
 * landmark store and the id is added there (an id beyond the store's id space is not), else frame2's depth point when it has one;
 * p2_1, p2_2, t_cam, cam, point1, point2 always; every other byte zero.  The records become the context's visual set exactly as
 * after velo_set_visual (velo_frame_to_frame[_batch], velo_register_batch and velo_get_good_matches work on it unchanged).
 * Outputs: n_per_cam [n_cams] (may be NULL) the matches of every camera; pairs_out [capacity][2] (may be NULL) the (point1, point2)
 * of the first `capacity` records; *n_out the total -- when it exceeds `capacity` the visual set is complete all the same.
 * VELO_ERR_STATE, with nothing changed: no velo_frames_reset, or a (frame, cam) of either frame that was never put.  Four launches,
 * one copy back (the chunk counts and 8 bytes per keypoint of frame2: the matches are not counted before it), one synchronisation; no cost depends on the size of the id space. */
int velo_build_matches(velo_ctx* ctx, int32_t frame1, int32_t frame2, const double* pose2_inv16 /* may be NULL */, int32_t* n_per_cam,
                       int32_t* pairs_out, int32_t capacity, int32_t* n_out);
/* The same for (frames1[i], frames2[i]) of ctxs[i], i < n_ctx, in the SAME four launches: a device table carries every context's
 * frames, slot tables, landmark store and pose, read per workgroup.  The rules of the other batch entries hold (distinct contexts on
 * one device, the first lends its stream and staging and waits for the others' streams, batch and single calls mix freely, n_ctx == 1
 * IS the single entry); contexts may differ in their camera counts and some may have no landmark store.  pose2_inv [n_ctx][16] or
 * NULL (no substitution anywhere); n_per_cam [n_ctx][8] (a context's first n_cams entries are written), pairs_out
 * [n_ctx][capacity][2], n_out [n_ctx].  Every context's visual set and outputs are byte-identical to the single entry's. */
int velo_build_matches_batch(velo_ctx** ctxs, int32_t n_ctx, const int32_t* frames1, const int32_t* frames2, const double* pose2_inv,
                             int32_t* n_per_cam, int32_t* pairs_out, int32_t capacity, int32_t* n_out);

/* --- the loop-closure edge: the same visual set joined by descriptors (main.cpp:359, velo.h:499-560) ------------------------------
 * The FREAK rows (n x 64 bytes, contiguous) of an entry velo_frames_put has made, kept on the device next to it in a second arena of
 * 64-byte rows with the keypoint arena's rules (geometric growth, first-fit free list, host directory; it starts at the byte count
 * velo_frames_reset was given for the keypoint arena, 1 MiB by default); nothing velo_frames_info reports changes.  A second call for
 * the same entry replaces the rows.  Refused before anything changes: VELO_ERR_INVALID when n differs from the entry's keypoint
 * count or rows is NULL with n > 0, VELO_ERR_STATE when the (frame, cam) was never put.  velo_frames_put on an entry DROPS its rows
 * (the keypoints they belonged to are gone), velo_frames_drop frees them with the frame, velo_frames_reset empties both arenas.
 * Asynchronous like velo_frames_put: one pinned upload, no synchronisation and no device allocation in the steady state. */
int velo_frames_put_descriptors(velo_ctx* ctx, int32_t frame, int32_t cam, const uint8_t* rows /* n x 64 */, int32_t n);
/* info[4] = (frame, cam) entries that hold rows, row-arena bytes (saturating at 2^31 - 1), row-arena reallocations, free row blocks. */
int velo_frames_desc_info(velo_ctx* ctx, int32_t* info);
/* velo_build_matches with matchFeatures in place of matchUsingId: per camera, in camera order, every row of frame1 (the query side,
 * the current frame) gets its nearest row of frame2 (the train side) by Hamming distance, the LOWEST train index on ties; min_dist is
 * the smallest distance of the camera and a match is dropped iff distance > max(1.5 min_dist, match_thresh), in double
 * (velo.h:536-549, exactly velo_match_descriptors' rules).  The kept pairs (point1, point2) = (queryIdx, trainIdx), query ascending,
 * give the records of velo_build_matches (id = frame2's id at point2, the same landmark substitution, every other byte zero); two
 * queries may keep one train row (two records); an empty side gives no match.  Arguments, outputs and the state the call leaves are
 * velo_build_matches' (capacity bounds pairs_out only; frame1's keypoint count bounds the matches).  VELO_ERR_STATE, with nothing
 * changed, also when a (frame, cam) of either frame holds no rows.  One upload of the call's tables, three launches on the resident
 * rows (int8-MFMA product, filter, record emit), one copy back (per camera min_dist and count, the pairs), one synchronisation: no
 * descriptor byte crosses the bus.  What this saves over velo_match_descriptors + host assembly + velo_set_visual has not been
 * measured yet (tools/loop_matches_bench.py is the measurement). */
int velo_build_matches_desc(velo_ctx* ctx, int32_t frame1, int32_t frame2, const double* pose2_inv16 /* may be NULL */, double match_thresh,
                            int32_t* n_per_cam, int32_t* pairs_out, int32_t capacity, int32_t* n_out);
/* The same for (frames1[i], frames2[i]) of ctxs[i] in the SAME three launches (every job carries the base pointers of its rows, so a
 * call names several contexts' arenas); the rules and the layout of the outputs are velo_build_matches_batch's. */
int velo_build_matches_desc_batch(velo_ctx** ctxs, int32_t n_ctx, const int32_t* frames1, const int32_t* frames2, const double* pose2_inv,
                                  double match_thresh, int32_t* n_per_cam, int32_t* pairs_out, int32_t capacity, int32_t* n_out);
/* The matches[cam].size() tests of main.cpp:366-371 for every loop-closure candidate of a frame: frame1's rows against those of
 * frames2[k], k < n_cand, camera by camera, in ONE launch set of n_cand x n_cams jobs on resident rows (frame1's are read in place by
 * every job).  n_kept / min_dist [n_cand][n_cams]: the pairs velo_build_matches_desc would keep and the camera's smallest distance
 * (-1: an empty side).  The visual set and everything else of the context stay as they are.  n_cand == 0 is valid (nothing is done).
 * VELO_ERR_STATE when a (frame, cam) was never put or holds no rows. */
int velo_match_frames(velo_ctx* ctx, int32_t frame1, const int32_t* frames2, int32_t n_cand, double match_thresh, int32_t* n_kept,
                      int32_t* min_dist);

/* --- pruning a resident frame to a registration's good matches (removeSlightlyLessTerribleFeatures, velo.h:272-327, main.cpp:504-514) ---
 * Read-back of one entry as the store holds it: *n / *n_with_depth its counts, *has_rows 1 when it holds descriptor rows; the first
 * `capacity` items of ids, keypoints_xy, has_depth and rows (64 bytes each) and the first `capacity_with_depth` depth points are
 * written; every array and every count may be NULL.  Synchronises.  VELO_ERR_STATE: no velo_frames_reset, or an entry never put. */
int velo_frames_get(velo_ctx* ctx, int32_t frame, int32_t cam, int32_t* ids, float* keypoints_xy /* n x 2 */, int32_t* has_depth,
                    float* kp_with_depth_xyz /* n_with_depth x 3 */, uint8_t* rows /* n x 64 */, int32_t capacity, int32_t capacity_with_depth,
                    int32_t* n, int32_t* n_with_depth, int32_t* has_rows);
/* Cuts ONE entry down to the SET of indices in keep_idx (any order, duplicates allowed: the std::set of velo.h:287-290), on the device,
 * exactly as velo.h:302-325 does: the kept keypoints stay in ascending old index; ids, keypoints and the descriptor rows (when the
 * entry holds rows) are gathered; has_depth[j] becomes the rank of j among the kept keypoints with depth, else -1; the new cloud is
 * old_cloud[old has_depth] in KEYPOINT order -- two keypoints that shared a depth point get a copy each, so the cloud can grow.  The
 * landmark store is untouched.  kept_out (may be NULL): the first `capacity` kept old indices, ascending; *n_kept / *n_with_depth (may
 * be NULL) the entry's new counts, which velo_frames_count reports from now on (the directory's largest id stays an upper bound).
 * n_keep == 0 empties the entry, which still counts as put.  This is how the result of a filter that stays on the host
 * (removeTerribleFeatures, velo.h:232-270) reaches the store: 4 bytes per kept keypoint instead of a second put of frame and rows.
 * Refused before anything changes: VELO_ERR_INVALID for an index outside [0, n) or a NULL list with n_keep > 0, VELO_ERR_STATE for an
 * entry never put.  One upload (the call's tables and the list), three launches (mark, count, move into scratch), one copy back (the
 * chunk counts and the kept indices), one synchronisation, then device-to-device copies of the result over the entry's block, queued
 * on the context's stream: no keypoint, depth point or descriptor byte crosses the bus, and no device allocation in the steady state. */
int velo_frames_keep(velo_ctx* ctx, int32_t frame, int32_t cam, const int32_t* keep_idx, int32_t n_keep, int32_t* kept_out, int32_t capacity,
                     int32_t* n_kept, int32_t* n_with_depth);
/* removeSlightlyLessTerribleFeatures(..., frame, good_matches) for every camera of `frame`, the keep set read on the device from the
 * context's visual set: keypoint i of camera cam stays iff some record with that cam and point1 == i has a non-zero gate flag in any
 * of its three slots -- exactly the point1 values velo_get_good_matches reports.  The result per camera is velo_frames_keep's.
 * n_kept / n_with_depth [n_cams] (may be NULL); kept_out [capacity] (may be NULL) the kept old indices, camera-major and ascending,
 * with which the caller compacts keypoints_p and whatever else it keeps; *n_out (may be NULL) their total.  The visual set and
 * velo_get_good_matches keep the OLD indices, as good_matches does in the reference.
 * The library must know that the visual set indexes these entries: velo_build_matches[_desc][_batch] record frame1 and a stamp of
 * each of its entries; velo_set_visual, a velo_frames_put / _keep / _prune / _drop of that frame and velo_frames_reset invalidate
 * them.  VELO_ERR_STATE, with nothing changed: no frame store; a camera of `frame` never put; `frame` is not the recorded frame1; a
 * stale stamp (so a second prune on one visual set); no registration or velo_build_visual since the build (the flags are not valid);
 * a sharded context (velo_set_query_shard / a communicator with world > 1), whose sweep covers a slice of the visual set only. */
int velo_frames_prune(velo_ctx* ctx, int32_t frame, int32_t* n_kept /* [n_cams] */, int32_t* n_with_depth /* [n_cams] */, int32_t* kept_out,
                      int32_t capacity, int32_t* n_out);
/* The same for (ctxs[i], frames[i]), i < n_ctx, in the SAME launches, under the rules of the other batch entries (distinct contexts on
 * one device, the first lends its stream, staging and scratch and waits for the others' streams, n_ctx == 1 IS the single entry,
 * camera counts may differ); n_kept / n_with_depth [n_ctx][8], kept_out [n_ctx][capacity], n_out [n_ctx].  No context changes when
 * one is refused.  Every context's entries and outputs are byte-identical to the single entry's. */
int velo_frames_prune_batch(velo_ctx** ctxs, int32_t n_ctx, const int32_t* frames, int32_t* n_kept, int32_t* n_with_depth, int32_t* kept_out,
                            int32_t capacity, int32_t* n_out);

/* --- a frame put with its keypoint depth computed on the device (velo.h:329-497 in front of the stores above) --------------------
 * One camera of a frame as the caller's extractor leaves it: ids and canonical keypoints, optionally the FREAK rows, and the camera's
 * window (velo_project_lidar's bounds). */
typedef struct velo_frame_cam {
    const int32_t* ids;          /* n */
    const float*   keypoints_xy; /* n x 2, canonical */
    const uint8_t* rows;         /* n x 64 FREAK rows, or NULL: the entry gets no rows */
    int32_t        n;
    double         bounds[4];    /* min_x, max_x, min_y, max_y of this camera: velo_project_lidar's */
} velo_frame_cam;

#define VELO_PUT_OBSERVE 1       /* also do velo_landmarks_observe for every camera, from the entry */

/* For every camera cam of the frame store (cams holds the store's n_cams entries) the end state of
 *     velo_project_lidar(ctx, of_target, the store's cam_trans[cam], bounds); velo_depth_association(keypoints, depth_assoc_thresh);
 *     velo_frames_put(frame, cam, ids, keypoints, has_depth, cloud); velo_frames_put_descriptors(frame, cam, rows, n) when rows is given;
 *     velo_landmarks_observe(frame, cam, the same arrays) with VELO_PUT_OBSERVE
 * byte for byte in velo_frames_get, velo_frames_info, velo_frames_desc_info (every block is placed at its exact size, in camera order)
 * and in the landmark store -- and has_depth and the depth cloud never exist on the host: the device projects the context's scan for
 * every camera into stacks of the frame store's own, associates depth, writes has_depth and the cloud (in keypoint order, from a scan:
 * no counter) into the entry and, on request, appends the landmark log from it.  The context's velo_project_lidar state
 * (velo_get_projection, velo_depth_association), the registration state, the visual set and the good matches are untouched; a recorded
 * frame1 stamp of `frame` is invalidated as by velo_frames_put.  n_with_depth [n_cams] (may be NULL): every camera's depth points.
 * Refused with nothing changed: VELO_ERR_INVALID for what velo_frames_put refuses (a negative id, an id >= 2^26, frame >= 2^22, a NULL
 * array with n > 0), for rows with n above the match key's row limit, for unknown flags and, with VELO_PUT_OBSERVE, for what
 * velo_landmarks_observe refuses (an id twice in one camera, a (frame, cam) observed before); VELO_ERR_STATE without a frame store,
 * without a cloud on the named side and, with VELO_PUT_OBSERVE, without a landmark store of the same camera count.
 * One upload (the call's tables, ids, keypoints and rows), four launches for all cameras (projection, depth search, chunk counts,
 * write; with VELO_PUT_OBSERVE one more that builds the log records, and the unchanged append per camera), one copy back (the chunk
 * counts), one synchronisation, then one device-to-device copy per block and row set: no keypoint or descriptor byte crosses the bus
 * twice, no has_depth or depth point crosses it at all, and no device allocation in the steady state.  What this saves over the four
 * calls per camera is measured by tools/frame_depth_bench.py. */
int velo_frames_put_frame(velo_ctx* ctx, int32_t frame, int32_t of_target, const velo_frame_cam* cams /* the store's n_cams */,
                          double depth_assoc_thresh, int32_t flags, int32_t* n_with_depth /* [n_cams], may be NULL */);
/* The same for (ctxs[i], frames[i], of_target[i]) in the SAME launches, under the rules of the other batch entries (distinct contexts
 * on one device, the first lends its stream, staging and scratch and waits for the others' streams, n_ctx == 1 IS the single entry);
 * contexts may differ in camera count, ring count and cloud size.  Every argument is checked before any context is touched, and no
 * context changes when one is refused.  Every context's stores are byte-identical to the single entry's. */
int velo_frames_put_frame_batch(velo_ctx** ctxs, int32_t n_ctx, const int32_t* frames, const int32_t* of_target,
                                const velo_frame_cam* cams /* [n_ctx][8], a context's first n_cams used */,
                                double depth_assoc_thresh, int32_t flags, int32_t* n_with_depth /* [n_ctx][8] */);

/* Read-back of the context's device-side visual set, whoever wrote it (velo_set_visual or velo_build_matches): *n = its records,
 * the first `capacity` are written (out may be NULL). */
int velo_get_visual(velo_ctx* ctx, velo_match* out, int32_t capacity, int32_t* n);

/* --- the sliding-window scan map of scan-to-map odometry, resident on the device ---------------------------------------------------
 * Scan-to-map (BASELINE configs 4-5) registers every scan against the last scans of the drive, all moved into one frame.  A map keeps
 * that window in HBM: every scan AS IT WAS REGISTERED, in its own sensor frame -- ring-major points, its ring offsets, a pose (row-major
 * 4 x 4, double) -- and writes the target cloud on demand in whatever reference frame the caller names.  So a map point is rounded to
 * float exactly once however long the drive runs, "everything in the newest pose's frame" is one streaming launch, and a pose can be
 * corrected afterwards (a loop closure) with no point traffic at all.  A map is owned like a scan cache: a handle of its own, bound to
 * one device, used with any context on that device, one call at a time.  It has no stream: insert and load run on the named context's
 * stream; a load on another stream waits (on the device) for the last insert, and an insert that may take a block a load still reads
 * waits for the last load.
 * create:   at most max_scans scans and max_points points (1 .. 2^30); VELO_ERR_NODEVICE without a device, as velo_cache_create.
 * insert:   the context's source cloud (of_target = 0) or whole-scan target cloud (1) enters under `frame`, device to device, with its
 *           ring offsets and pose16.  Empty rings of a source are not stored as rings (a target ring may not be empty).  Before the scan
 *           is stored the OLDEST scans go while the map holds max_scans scans or points + n > max_points; *n_evicted (may be NULL) says
 *           how many.  Refused with nothing changed and nothing evicted: VELO_ERR_STATE for what velo_cache_store refuses (no scan on
 *           that side, a target shard) and for a frame that is present (drop it first); VELO_ERR_INVALID for a context on another
 *           device, a scan with no point, a scan of more than max_points points, a pose that is not finite.  Storage is one arena of
 *           points with a first-fit free list (blocks are neither split nor merged: made for a window of scans of similar size); it
 *           starts at 4 KB and grows geometrically, and growth is the only wait: in the steady state an insert is one asynchronous
 *           copy, no device allocation, no synchronisation.
 * set_pose: replaces a scan's pose.  drop / clear: the blocks return to the free list.  All three are host bookkeeping;
 *           VELO_ERR_STATE for a frame that is not in the map.
 * frames:   oldest first; returns the count (0 for NULL).
 * info:     int64[8] = scans, points, rings, max_scans, max_points, evictions so far, arena capacity in points, arena growths.
 * get_scan: one stored scan back (tests): *n_points / *n_rings always; the first capacity_points points (n x 3), the first
 *           capacity_rings entries of its n_rings + 1 ring offsets, its pose; any output may be NULL.
 * load:     the map becomes the context's target in the frame ref_inv16 -- the caller supplies the INVERSE of the reference pose, as
 *           for velo_landmarks_at_frame.  Scans oldest first, rings in scan order, ring offsets concatenated.  Per scan the host forms
 *           M = ref_inv * pose in double, every entry of rows 0..2 as ((a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j) + a_i3 b_3j; per point the
 *           device computes q_i = ((M_i0 x + M_i1 y) + M_i2 z) + M_i3 with the floats widened to double, summed left to right without
 *           contraction, and rounds to float.  No division by a fourth row; no shortcut for an identity (-0.0f comes out +0.0f).  The
 *           end state is the one velo_set_target leaves when handed that cloud and those offsets, byte for byte: cloud, ring ids, padded
 *           rings, bounding box and index; correspondences, partials and warm-start seeds invalidated; the target owned by the context
 *           (velo_share_target from it works).  One table upload and ONE materialise launch for the whole window, then the ingest launch
 *           of velo_set_target on the materialised cloud in place, then the index build.  VELO_ERR_STATE for an empty map, with the
 *           context untouched.
 * load_batch: entry i makes maps[i] the target of ctxs[i] in the frame ref_inv[16 i ..]: distinct contexts on one device (the rules of
 *           the other batch entries: the first lends its stream and waits for the others' streams; n == 1 IS the single entry); two
 *           entries may name one map with different frames.  One table upload and one materialise launch for every scan of every entry,
 *           then every context's ingest and bounding-box request are enqueued before any is waited for.  Every argument and every map
 *           is checked before any context is touched.  Every context's end state is byte-identical to the single entry's. */
typedef struct velo_map velo_map;
int velo_map_create(velo_map** out, int32_t device, int32_t max_scans, int64_t max_points);
int velo_map_destroy(velo_map* map);                      /* NULL is fine */
int velo_map_insert(velo_map* map, velo_ctx* ctx, int32_t of_target, int32_t frame, const double pose16[16], int32_t* n_evicted);
int velo_map_set_pose(velo_map* map, int32_t frame, const double pose16[16]);
int velo_map_drop(velo_map* map, int32_t frame);
int velo_map_clear(velo_map* map);
int velo_map_frames(const velo_map* map, int32_t* frames_out, int32_t capacity);
int velo_map_info(const velo_map* map, int64_t* info /* [8] */);
int velo_map_get_scan(velo_map* map, int32_t frame, float* xyz /* n x 3 */, int32_t capacity_points, int32_t* n_points,
                      int32_t* ring_offsets, int32_t capacity_rings, int32_t* n_rings, double pose16[16]);
int velo_map_load(velo_map* map, velo_ctx* ctx, const double ref_inv16[16]);
int velo_map_load_batch(velo_map** maps, velo_ctx** ctxs, int32_t n, const double* ref_inv /* n x 16 */);

#ifdef __cplusplus
}
#endif
#endif /* VELO_HIP_H_ */
