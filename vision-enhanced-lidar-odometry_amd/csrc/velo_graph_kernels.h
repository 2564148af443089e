// velo_graph_kernels.h -- the batch optimisation of a drive's pose graph (reference main.cpp:190-204 the prior, main.cpp:516-536 the
// Pose3d_Pose3d factors, main.cpp:728-745 the solve).  Included by velo_hip.hip (declarations) and by velo_unit_graph.hip
// (VELO_DEF_GRAPH: the definitions); gfx950 only.
//
// A node is the 6 doubles (angle-axis, translation) of a frame's world pose T; an edge (from, to, z, info) states T_to = T_from Z and
// its residual is sqrt(info) * pose_vec(Z^-1 T_from^-1 T_to), the angle-axis of the rotation and then the translation (the form of
// main.cpp:416-424).  Fixed nodes are constants.  The solver is the trust-region Levenberg-Marquardt of SURVEY.md B1 over the free
// nodes (the controller of velo_trust_region.h, run by the host); its linear step is a block-Jacobi preconditioned conjugate gradient on the damped, Jacobi-scaled normal equations
//     (c H c + D / mu) y = -c g,      H = J^T J block-sparse: a 6 x 6 diagonal block per free node, one off-diagonal block per edge,
// whose matrix is never assembled: a product gathers, per node, the node's diagonal block and the A^T B block of every incident edge.
//     graph_linearize_kernel  one thread per edge: residual, the two 6 x 6 Jacobians, A^T A, B^T B, A^T B, A^T r, B^T r, the cost term
//     graph_linearize_weighted_kernel  the same for a store that holds a 6 x 6 information or a Cauchy loss on some edge: whitens
//                             with the information's Cholesky factor, scales by rho'
//     graph_assemble_kernel   one thread per free node, over its incident edges in the host's fixed order: diagonal block, gradient,
//                             at the start the Jacobi scale
//     graph_cg_begin_kernel   one thread per free node: D, the Cholesky of the damped preconditioner block, y = 0, r = b, z = M^-1 r
//     graph_cg_ap_kernel      CG, first half of iteration k:  beta, p = z + beta p, q = A p (the gather), partial sums of p.q
//     graph_cg_update_kernel  CG, second half:  alpha, y += alpha p, r -= alpha q, z = M^-1 r, partial sums of r.z
//     graph_step_kernel       one thread per free node: candidate pose, the node's share of the model change and of |step|^2
//     graph_reduce_kernel     one workgroup per scalar: cost over edges; model change, |step|^2, |x|^2, gradient maximum over nodes
// A dot product is one partial sum per workgroup (a fixed tree), and the NEXT launch adds the partial sums in a fixed order in every
// workgroup: no atomics on sums, no grid-wide barrier, no workgroup waits for another.  The stopping test of CG is evaluated by
// every workgroup on the same numbers; once it holds, the launches that were enqueued behind it return at once.  The host enqueues
// iterations in batches and reads one GraphRecord per batch, and one per LM iteration, from which it takes the LM decision.
// A call may select the envelope solver for the linear step instead (velo_graph_params.reserved[0]): the same system, assembled as a
// block skyline and factored exactly -- graph_env_fill_kernel, graph_env_factor_kernel, graph_env_solve_kernel at the end of this file.
// velo_graph_covariance reads blocks of (J^T J)^-1 off the same factor of the undamped system: graph_env_fill_undamped_kernel,
// graph_env_selinv_kernel, graph_env_column_kernel, graph_cov_gather_kernel behind them.  velo_graph_edge_gate and
// velo_graph_loop_candidates turn those blocks into the covariance of a relative pose in an edge's tangent space: graph_env_column_full_kernel,
// graph_relcov_kernel, graph_loop_candidates_kernel, graph_loop_compact_kernel at the very end.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/velo_hip.h"
#include "velo_scan_types.h"
#include "velo_device_math.h"

#ifndef VELO_DEF_GRAPH
#define VELO_DEF_GRAPH 0
#endif

namespace velo {

constexpr int kGrBlk = 91;                       // per edge: upper A^T A (21), upper B^T B (21), A^T B (36), A^T r (6), B^T r (6), cost
constexpr int kGrAtA = 0, kGrBtB = 21, kGrAtB = 42, kGrAtr = 78, kGrBtr = 84, kGrCost = 90;
constexpr int kGrNode = 27;                      // per free node: upper diagonal block (21), gradient (6)
constexpr int kGrThreads = 64;                   // threads of a workgroup of the per-node and per-edge kernels
constexpr int kGrRed = 5;                        // cost, model change, |step|^2, |x|^2, gradient maximum

struct GraphRecord {                             // what the host reads: 80 bytes
    double red[kGrRed];
    double cg_rel;                               // sqrt(rho_k / rho_0) when CG stopped
    int cg_done, cg_iters, bad, pad;
    double pad2[2];
};

struct GraphArgs {
    // the store
    const int* from; const int* to;              // [E]
    const double* z; const double* info;         // [E][6], [E]
    double* x;                                   // [2][x_stride]: poses by frame number, current / candidate
    size_t x_stride;
    // the call
    const int* node;                             // [n_free] -> frame
    const int* inc_start;                        // [n_free + 1]
    const int* inc;                              // incident edges of a node, ascending: 2 edge + (1 if the node is the edge's `to`)
    const int* inc_other;                        // beside inc: the free index of the edge's other end, -1 when that is a constant (so
                                                 // the gather of a product has no chain of dependent loads edge -> frame -> index)
    double* blk;                                 // [2][E][91]
    double* nd;                                  // [2][n_free][27]
    double* scale; double* diag;                 // [n_free][6]
    double* chol;                                // [n_free][21]: lower triangle, row-major
    double* y; double* r; double* zv; double* q; double* p;     // [n_free][6] each; p: [2][n_free][6]
    double* part_rho0; double* part_rho; double* part_sigma;    // [nb], [2][nb], [nb]
    double* nterm;                               // [n_free][2]: model change, |step|^2
    GraphRecord* rec;
    int E, n_free, nb;
    double cg_tol2;
    LMParams lm;
    // the envelope solver (null for a CG call): the order of the free nodes and the block skyline in it
    const int* env_perm;                         // [n_free]: position -> free index
    const int* env_pos;                          // [n_free]: free index -> position
    const int* env_first;                        // [n_free]: the first column of row i (a position)
    const int* env_rowptr;                       // [n_free + 1]: row i holds the blocks of columns first(i) .. i from here, in blocks
    const int* env_last;                         // [n_free]: the last row with first <= k, what elimination step k reaches
    double* env;                                 // [blocks][36], row-major 6 x 6
};

// What a weighted store has beside GraphArgs (null for a scalar one): matrix information and robust losses.  An argument of its own,
// of graph_linearize_weighted_kernel alone: every graph kernel takes GraphArgs by value, and the CG path is 200,000 launches per call on
// a drive -- with these 24 bytes inside GraphArgs that path measured 1 to 2 % slower for a store that has no use for them.
struct GraphWeights {
    const double* winfo;                         // [E][21]: the Cholesky factor L of W = L L^T, lower triangle, row-major packed
    const double* loss;                          // [E]: 0 = trivial, a > 0 = Cauchy(a) on s = r^T W r
    double* estat;                               // [2][E][2]: s and rho'(s) of the last linearisation of each buffer
};

__device__ __forceinline__ int graph_lower6(int i, int j) { return (i * (i + 1)) / 2 + j; }                      // j <= i

// R(w) and the left Jacobian J_l(w), R(w + d) = Exp(J_l d) R(w) to first order: column j of J_l is the axial vector of (dR / dw_j) R^T,
// with dR / dw from the dual-number rotation of the three unit vectors (velo_device_math.h)
__device__ __forceinline__ void graph_rot(const double w[3], double R[9], double Jl[9]) {
    PoseRot P;
    pose_rot_init(w, &P);
    double dR[3][9];
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
        D3 c[3];
        rotate_point(P, e, c);
#pragma unroll
        for (int i = 0; i < 3; i++) {
            R[i * 3 + k] = c[i].a;
#pragma unroll
            for (int j = 0; j < 3; j++) dR[j][i * 3 + k] = c[i].v[j];
        }
    }
#pragma unroll
    for (int j = 0; j < 3; j++) {
        double S[9];
#pragma unroll
        for (int a = 0; a < 3; a++) {
#pragma unroll
            for (int b = 0; b < 3; b++) S[a * 3 + b] = dR[j][a * 3] * R[b * 3] + dR[j][a * 3 + 1] * R[b * 3 + 1] + dR[j][a * 3 + 2] * R[b * 3 + 2];
        }
        Jl[0 * 3 + j] = 0.5 * (S[7] - S[5]);
        Jl[1 * 3 + j] = 0.5 * (S[2] - S[6]);
        Jl[2 * 3 + j] = 0.5 * (S[3] - S[1]);
    }
}

__device__ __forceinline__ void graph_rot_value(const double w[3], double R[9]) {
    PoseRot P;
    pose_rot_init(w, &P);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
        double c[3];
        rotate_point_value(P, e, c);
        R[k] = c[0]; R[3 + k] = c[1]; R[6 + k] = c[2];
    }
}

// ceres::RotationMatrixToAngleAxis: through the quaternion (RotationMatrixToQuaternion, QuaternionToAngleAxis), angle in [0, pi]
__device__ __forceinline__ void graph_log(const double R[9], double phi[3]) {
    const double tr = R[0] + R[4] + R[8];
    double q0, q1, q2, q3;
    if (tr >= 0.0) {
        double t = sqrt(tr + 1.0);
        q0 = 0.5 * t; t = 0.5 / t;
        q1 = (R[7] - R[5]) * t; q2 = (R[2] - R[6]) * t; q3 = (R[3] - R[1]) * t;
    } else if (R[0] >= R[4] && R[0] >= R[8]) {
        double t = sqrt(R[0] - R[4] - R[8] + 1.0);
        q1 = 0.5 * t; t = 0.5 / t;
        q0 = (R[7] - R[5]) * t; q2 = (R[3] + R[1]) * t; q3 = (R[6] + R[2]) * t;
    } else if (R[4] >= R[8]) {
        double t = sqrt(R[4] - R[8] - R[0] + 1.0);
        q2 = 0.5 * t; t = 0.5 / t;
        q0 = (R[2] - R[6]) * t; q3 = (R[7] + R[5]) * t; q1 = (R[1] + R[3]) * t;
    } else {
        double t = sqrt(R[8] - R[0] - R[4] + 1.0);
        q3 = 0.5 * t; t = 0.5 / t;
        q0 = (R[3] - R[1]) * t; q1 = (R[2] + R[6]) * t; q2 = (R[5] + R[7]) * t;
    }
    const double s2 = q1 * q1 + q2 * q2 + q3 * q3;
    double k = 2.0;
    if (s2 > 0.0) {
        const double s = sqrt(s2);
        const double two_theta = 2.0 * (q0 < 0.0 ? atan2(-s, -q0) : atan2(s, q0));
        k = two_theta / s;
    }
    phi[0] = q1 * k; phi[1] = q2 * k; phi[2] = q3 * k;
}

// the inverse right Jacobian, Log(R Exp(e)) = phi + J_r^-1(phi) e to first order: I + K / 2 + (1 / t^2 - cot(t / 2) / (2 t)) K^2
__device__ __forceinline__ void graph_jr_inv(const double phi[3], double J[9]) {
    const double t2 = phi[0] * phi[0] + phi[1] * phi[1] + phi[2] * phi[2];
    double coef;
    if (t2 > 1e-6) {
        const double t = sqrt(t2);
        double sh, ch;
        velo_sincos(0.5 * t, &sh, &ch);
        coef = 1.0 / t2 - ch / (2.0 * t * sh);
    } else {
        coef = 1.0 / 12.0 + t2 / 720.0;
    }
    const double x = phi[0], y = phi[1], z = phi[2];
    // K = [phi]x, K^2 = phi phi^T - t2 I
    J[0] = 1.0 + coef * (x * x - t2); J[1] = -0.5 * z + coef * x * y;       J[2] = 0.5 * y + coef * x * z;
    J[3] = 0.5 * z + coef * x * y;    J[4] = 1.0 + coef * (y * y - t2);     J[5] = -0.5 * x + coef * y * z;
    J[6] = -0.5 * y + coef * x * z;   J[7] = 0.5 * x + coef * y * z;        J[8] = 1.0 + coef * (z * z - t2);
}

__device__ __forceinline__ void graph_mul3(const double A[9], const double B[9], double C[9]) {           // C = A B
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) C[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
    }
}
__device__ __forceinline__ void graph_mul3_tn(const double A[9], const double B[9], double C[9]) {        // C = A^T B
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) C[i * 3 + j] = A[i] * B[j] + A[3 + i] * B[3 + j] + A[6 + i] * B[6 + j];
    }
}
__device__ __forceinline__ void graph_mul3_tt(const double A[9], const double B[9], double C[9]) {        // C = A^T B^T
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) C[i * 3 + j] = A[i] * B[j * 3] + A[3 + i] * B[j * 3 + 1] + A[6 + i] * B[j * 3 + 2];
    }
}

// ---- linearise: one thread per edge, at the poses of buffer `which` -------------------------------------------------------------
// the unweighted residual r = pose_vec(Z^-1 T_from^-1 T_to) of edge e and its Jacobians A (from), B (to), row-major 6 x 6: the text both
// linearise kernels share, and graph_relcov_kernel and graph_loop_candidates_kernel with them.  xf, xt: the 6 doubles of the two poses; zz: of Z
__device__ __forceinline__ void graph_edge_terms_at(const double* xf, const double* xt, const double* zz, double r[6], double A[36], double B[36]) {
    const double wf[3] = {xf[0], xf[1], xf[2]}, wt[3] = {xt[0], xt[1], xt[2]}, wz[3] = {zz[0], zz[1], zz[2]};
    double Rf[9], Jlf[9], Rt[9], Jlt[9], Rz[9];
    graph_rot(wf, Rf, Jlf);
    graph_rot(wt, Rt, Jlt);
    graph_rot_value(wz, Rz);
    double Q[9], RE[9], phi[3], Ji[9];
    graph_mul3_tt(Rz, Rf, Q);                                         // Rz^T Rf^T
    graph_mul3(Q, Rt, RE);
    graph_log(RE, phi);
    graph_jr_inv(phi, Ji);
    const double d[3] = {xt[3] - xf[3], xt[4] - xf[4], xt[5] - xf[5]};
#pragma unroll
    for (int i = 0; i < 3; i++) {
        r[i] = phi[i];
        r[3 + i] = (Q[i * 3] * d[0] + Q[i * 3 + 1] * d[1] + Q[i * 3 + 2] * d[2]) - (Rz[i] * zz[3] + Rz[3 + i] * zz[4] + Rz[6 + i] * zz[5]);
    }
    // A = d r / d x_from = [-Ji Rt^T Jl(wf), 0; Q [d]x Jl(wf), -Q],  B = d r / d x_to = [Ji Rt^T Jl(wt), 0; 0, Q]
    double T[9], U[9];
    graph_mul3_tn(Rt, Jlf, T);
    graph_mul3(Ji, T, U);
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) { A[i * 6 + j] = -U[i * 3 + j]; A[i * 6 + 3 + j] = 0.0; A[(3 + i) * 6 + 3 + j] = -Q[i * 3 + j]; }
    }
    const double Dx[9] = {0.0, -d[2], d[1], d[2], 0.0, -d[0], -d[1], d[0], 0.0};
    graph_mul3(Dx, Jlf, T);
    graph_mul3(Q, T, U);
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) A[(3 + i) * 6 + j] = U[i * 3 + j];
    }
    graph_mul3_tn(Rt, Jlt, T);
    graph_mul3(Ji, T, U);
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) { B[i * 6 + j] = U[i * 3 + j]; B[i * 6 + 3 + j] = 0.0; B[(3 + i) * 6 + j] = 0.0; B[(3 + i) * 6 + 3 + j] = Q[i * 3 + j]; }
    }
}
// edge e of the store at the poses of buffer `which`
__device__ __forceinline__ void graph_edge_terms(const GraphArgs& G, int e, int which, double r[6], double A[36], double B[36]) {
    graph_edge_terms_at(G.x + (size_t)which * G.x_stride + (size_t)G.from[e] * 6, G.x + (size_t)which * G.x_stride + (size_t)G.to[e] * 6,
                        G.z + (size_t)e * 6, r, A, B);
}

// w A^T A, w B^T B (upper), w A^T B, w A^T r, w B^T r into the edge's block
__device__ __forceinline__ void graph_edge_products(double* out, const double A[36], const double B[36], const double r[6], double w) {
#pragma unroll
    for (int a = 0; a < 6; a++) {
#pragma unroll
        for (int b = 0; b < 6; b++) {
            double ab = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) ab += A[k * 6 + a] * B[k * 6 + b];
            out[kGrAtB + a * 6 + b] = w * ab;
            if (b >= a) {
                double aa = 0.0, bb = 0.0;
#pragma unroll
                for (int k = 0; k < 6; k++) { aa += A[k * 6 + a] * A[k * 6 + b]; bb += B[k * 6 + a] * B[k * 6 + b]; }
                out[kGrAtA + upper6(a, b)] = w * aa;
                out[kGrBtB + upper6(a, b)] = w * bb;
            }
        }
        double ar = 0.0, br = 0.0;
#pragma unroll
        for (int k = 0; k < 6; k++) { ar += A[k * 6 + a] * r[k]; br += B[k * 6 + a] * r[k]; }
        out[kGrAtr + a] = w * ar;
        out[kGrBtr + a] = w * br;
    }
}

__global__ void __launch_bounds__(kGrThreads)
graph_linearize_kernel(GraphArgs G, int which)
#if VELO_DEF_GRAPH
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G.E) return;
    double r[6], A[36], B[36];
    graph_edge_terms(G, e, which, r, A, B);
    const double w = G.info[e];
    double* out = G.blk + ((size_t)which * G.E + e) * kGrBlk;
    graph_edge_products(out, A, B, r, w);
    double rr = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) rr += r[k] * r[k];
    out[kGrCost] = 0.5 * (w * rr);
}
#else
;
#endif

// The same for a store with matrix information and robust losses (velo_graph_add_edges_weighted).  winfo holds per edge the Cholesky
// factor L of its information W = L L^T (lower triangle, row-major packed).  The thread whitens in place, rows ascending -- row i of
// L^T A needs the rows >= i only, so no second 6 x 6 is alive --: A <- L^T A, B <- L^T B, r <- L^T r; then s = |r|^2 = r^T W r, the
// loss rho(s) = s (loss 0) or a^2 ln(1 + s / a^2) (Cauchy(a), ceres::CauchyLoss), and the products above with w = rho'(s): Ceres'
// corrector with alpha = 0, which is exact for a loss whose second derivative is negative.  Every sum has a fixed order.  (s, rho') go
// to estat for velo_graph_edge_stats.
__global__ void __launch_bounds__(kGrThreads)
graph_linearize_weighted_kernel(GraphArgs G, GraphWeights Wt, int which)
#if VELO_DEF_GRAPH
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= G.E) return;
    double r[6], A[36], B[36];
    graph_edge_terms(G, e, which, r, A, B);
    const double* Lp = Wt.winfo + (size_t)e * 21;
    double L[21];
#pragma unroll
    for (int a = 0; a < 21; a++) L[a] = Lp[a];
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int c = 0; c < 6; c++) {
            double sa = 0.0, sb = 0.0;
#pragma unroll
            for (int k = i; k < 6; k++) { sa += L[graph_lower6(k, i)] * A[k * 6 + c]; sb += L[graph_lower6(k, i)] * B[k * 6 + c]; }
            A[i * 6 + c] = sa;
            B[i * 6 + c] = sb;
        }
        double sr = 0.0;
#pragma unroll
        for (int k = i; k < 6; k++) sr += L[graph_lower6(k, i)] * r[k];
        r[i] = sr;
    }
    double s = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) s += r[k] * r[k];
    const double a = Wt.loss[e];
    double rho = s, w = 1.0;
    if (a > 0.0) {
        const double b = a * a, t = 1.0 + s / b;
        rho = b * log(t);
        w = 1.0 / t;
    }
    double* out = G.blk + ((size_t)which * G.E + e) * kGrBlk;
    graph_edge_products(out, A, B, r, w);
    out[kGrCost] = 0.5 * rho;
    double* st = Wt.estat + ((size_t)which * G.E + e) * 2;
    st[0] = s;
    st[1] = w;
}
#else
;
#endif

// a scalar edge in a weighted store: W = info I, that is L = sqrt(info) I, and the trivial loss; one thread per edge of [first, first + n)
__global__ void __launch_bounds__(kGrThreads)
graph_promote_kernel(const double* info, double* winfo, double* loss, int first, int n)
#if VELO_DEF_GRAPH
{
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const size_t e = (size_t)first + (size_t)k;
    const double l = sqrt(info[e]);
#pragma unroll
    for (int i = 0; i < 6; i++) {
#pragma unroll
        for (int j = 0; j <= i; j++) winfo[e * 21 + graph_lower6(i, j)] = i == j ? l : 0.0;
    }
    loss[e] = 0.0;
}
#else
;
#endif

// ---- assemble: one thread per free node, its incident edges in the list's order ----------------------------------------------
// mode 0: the start of a call, which also fixes the Jacobi scaling (B1: once)
__global__ void __launch_bounds__(kGrThreads)
graph_assemble_kernel(GraphArgs G, int which, int mode)
#if VELO_DEF_GRAPH
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= G.n_free) return;
    double acc[kGrNode];
#pragma unroll
    for (int a = 0; a < kGrNode; a++) acc[a] = 0.0;
    const int end = G.inc_start[i + 1];
    for (int k = G.inc_start[i]; k < end; k++) {
        const int code = G.inc[k];
        const double* b = G.blk + ((size_t)which * G.E + (code >> 1)) * kGrBlk;
        const double* H = b + ((code & 1) ? kGrBtB : kGrAtA);
        const double* g = b + ((code & 1) ? kGrBtr : kGrAtr);
#pragma unroll
        for (int a = 0; a < 21; a++) acc[a] += H[a];
#pragma unroll
        for (int a = 0; a < 6; a++) acc[21 + a] += g[a];
    }
    double* out = G.nd + ((size_t)which * G.n_free + i) * kGrNode;
#pragma unroll
    for (int a = 0; a < kGrNode; a++) out[a] = acc[a];
    if (mode == 0) {
#pragma unroll
        for (int a = 0; a < 6; a++) G.scale[(size_t)i * 6 + a] = 1.0 / (1.0 + sqrt(acc[upper6(a, a)]));
    }
}
#else
;
#endif

// ---- sums ------------------------------------------------------------------------------------------------------------------
// one value per thread of a 64-thread workgroup -> their sum, by a fixed tree
__device__ __forceinline__ double graph_block_sum(double* buf, double v) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int s = kGrThreads / 2; s > 0; s >>= 1) {
        if (t < s) buf[t] += buf[t + s];
        __syncthreads();
    }
    const double out = buf[0];
    __syncthreads();
    return out;
}
// the partial sums of a previous launch, added in the same order by every workgroup
__device__ __forceinline__ double graph_parts_sum(double* buf, const double* part, int nb) {
    double acc = 0.0;
    for (int k = threadIdx.x; k < nb; k += kGrThreads) acc += part[k];
    return graph_block_sum(buf, acc);
}

// the record's CG words, read by one thread for the whole workgroup: bit 0 = CG has stopped, bit 1 = the step is invalid
__device__ __forceinline__ int graph_cg_flags(const GraphRecord* rec) {
    __shared__ int flags_s;
    if (threadIdx.x == 0) flags_s = (rec->cg_done != 0 ? 1 : 0) | (rec->bad != 0 ? 2 : 0);
    __syncthreads();
    const int f = flags_s;
    __syncthreads();
    return f;
}

// L L^T = M for a 6 x 6 block in registers; L overwrites the lower triangle
__device__ __forceinline__ bool graph_chol6(double M[36]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double dj = M[j * 6 + j];
#pragma unroll
        for (int k = 0; k < j; k++) dj -= M[j * 6 + k] * M[j * 6 + k];
        if (!(dj > 0.0) || !isfinite(dj)) { ok = false; dj = 1.0; }
        const double l = sqrt(dj);
        M[j * 6 + j] = l;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double s = M[i * 6 + j];
#pragma unroll
            for (int k = 0; k < j; k++) s -= M[i * 6 + k] * M[j * 6 + k];
            M[i * 6 + j] = s / l;
        }
    }
    return ok;
}
// L L^T v = b with the packed lower triangle
__device__ __forceinline__ void graph_chol_solve(const double* L, const double b[6], double v[6]) {
    double t[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; k++) s -= L[graph_lower6(i, k)] * t[k];
        t[i] = s / L[graph_lower6(i, i)];
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double s = t[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) s -= L[graph_lower6(k, i)] * v[k];
        v[i] = s / L[graph_lower6(i, i)];
    }
}

// (c H_ii c) v for the node's upper-packed diagonal block
__device__ __forceinline__ void graph_diag_mul(const double* H, const double c[6], const double v[6], double out[6]) {
#pragma unroll
    for (int a = 0; a < 6; a++) {
        double s = 0.0;
#pragma unroll
        for (int b = 0; b < 6; b++) s += H[upper6(a < b ? a : b, a < b ? b : a)] * (c[b] * v[b]);
        out[a] = c[a] * s;
    }
}

// ---- CG ---------------------------------------------------------------------------------------------------------------------
// The start of an LM iteration's linear solve at buffer `cur`: D (refreshed after an accepted step), M_i = c H_ii c + D_i / mu and its
// Cholesky, b = -c g, y = 0, r = b, z = M^-1 r, the partial sums of rho_0 = r.z.  The host has cleared the record's CG words before.
__global__ void __launch_bounds__(kGrThreads)
graph_cg_begin_kernel(GraphArgs G, int cur, double mu, int refresh)
#if VELO_DEF_GRAPH
{
    __shared__ double buf[kGrThreads];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double rz = 0.0;
    if (i < G.n_free) {
        const double* nd = G.nd + ((size_t)cur * G.n_free + i) * kGrNode;
        double c[6], M[36], b[6], z[6];
#pragma unroll
        for (int a = 0; a < 6; a++) c[a] = G.scale[(size_t)i * 6 + a];
#pragma unroll
        for (int a = 0; a < 6; a++) {
#pragma unroll
            for (int bb = 0; bb < 6; bb++) M[a * 6 + bb] = nd[upper6(a < bb ? a : bb, a < bb ? bb : a)] * c[a] * c[bb];
        }
#pragma unroll
        for (int a = 0; a < 6; a++) {
            double dg = G.diag[(size_t)i * 6 + a];
            if (refresh) { dg = fmin(fmax(M[a * 6 + a], G.lm.min_diag), G.lm.max_diag); G.diag[(size_t)i * 6 + a] = dg; }
            M[a * 6 + a] += dg / mu;
            b[a] = -(nd[21 + a] * c[a]);
        }
        if (!graph_chol6(M)) atomicOr(&G.rec->bad, 1);
        double L[21];
#pragma unroll
        for (int a = 0; a < 6; a++) {
#pragma unroll
            for (int bb = 0; bb <= a; bb++) { L[graph_lower6(a, bb)] = M[a * 6 + bb]; G.chol[(size_t)i * 21 + graph_lower6(a, bb)] = M[a * 6 + bb]; }
        }
        graph_chol_solve(L, b, z);
#pragma unroll
        for (int a = 0; a < 6; a++) {
            G.y[(size_t)i * 6 + a] = 0.0;
            G.r[(size_t)i * 6 + a] = b[a];
            G.zv[(size_t)i * 6 + a] = z[a];
            rz += b[a] * z[a];
        }
    }
    const double s = graph_block_sum(buf, rz);
    if (threadIdx.x == 0) { G.part_rho0[blockIdx.x] = s; G.part_rho[blockIdx.x] = s; }
}
#else
;
#endif

// First half of CG iteration k.  rho_k lies in part_rho[k & 1], rho_(k-1) in the other half.  Stops -- and lets every later launch
// return at once -- when rho_k <= tol^2 rho_0.  p_(k-1) is read from p[k & 1] and p_k written to p[(k + 1) & 1]: a neighbour's p_k is
// recomputed from its z and p_(k-1), so no thread reads what another writes in this launch.
__global__ void __launch_bounds__(kGrThreads)
graph_cg_ap_kernel(GraphArgs G, int k, int cur, double mu)
#if VELO_DEF_GRAPH
{
    __shared__ double buf[kGrThreads];
    const int flags = graph_cg_flags(G.rec);
    if (flags & 1) return;
    const double rho = graph_parts_sum(buf, G.part_rho + (size_t)(k & 1) * G.nb, G.nb);
    const double rho0 = graph_parts_sum(buf, G.part_rho0, G.nb);
    if ((flags & 2) || !(rho > G.cg_tol2 * rho0)) {               // (also ends on a NaN)
        if (blockIdx.x == 0 && threadIdx.x == 0) { G.rec->cg_iters = k; G.rec->cg_rel = rho0 > 0.0 ? sqrt(rho / rho0) : 0.0; G.rec->cg_done = 1; }
        return;
    }
    double beta = 0.0;
    if (k > 0) beta = rho / graph_parts_sum(buf, G.part_rho + (size_t)((k & 1) ^ 1) * G.nb, G.nb);
    const size_t n6 = (size_t)G.n_free * 6;
    const double* p_old = G.p + (size_t)(k & 1) * n6;
    double* p_new = G.p + (size_t)((k + 1) & 1) * n6;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double pq = 0.0;
    if (i < G.n_free) {
        double c[6], p[6], q[6];
#pragma unroll
        for (int a = 0; a < 6; a++) {
            c[a] = G.scale[(size_t)i * 6 + a];
            p[a] = G.zv[(size_t)i * 6 + a];
            if (k > 0) p[a] += beta * p_old[(size_t)i * 6 + a];
            p_new[(size_t)i * 6 + a] = p[a];
        }
        graph_diag_mul(G.nd + ((size_t)cur * G.n_free + i) * kGrNode, c, p, q);
#pragma unroll
        for (int a = 0; a < 6; a++) q[a] += (G.diag[(size_t)i * 6 + a] / mu) * p[a];
        const int end = G.inc_start[i + 1];
        for (int m = G.inc_start[i]; m < end; m++) {
            const int code = G.inc[m], e = code >> 1, side = code & 1;
            const int j = G.inc_other[m];
            if (j < 0) continue;                                      // the other end is a constant
            double v[6];
#pragma unroll
            for (int a = 0; a < 6; a++) {
                double pj = G.zv[(size_t)j * 6 + a];
                if (k > 0) pj += beta * p_old[(size_t)j * 6 + a];
                v[a] = G.scale[(size_t)j * 6 + a] * pj;
            }
            const double* W = G.blk + ((size_t)cur * G.E + e) * kGrBlk + kGrAtB;
#pragma unroll
            for (int a = 0; a < 6; a++) {
                double s = 0.0;
#pragma unroll
                for (int b = 0; b < 6; b++) s += (side ? W[b * 6 + a] : W[a * 6 + b]) * v[b];
                q[a] += c[a] * s;
            }
        }
#pragma unroll
        for (int a = 0; a < 6; a++) { G.q[(size_t)i * 6 + a] = q[a]; pq += p[a] * q[a]; }
    }
    const double s = graph_block_sum(buf, pq);
    if (threadIdx.x == 0) G.part_sigma[blockIdx.x] = s;
}
#else
;
#endif

// Second half of CG iteration k: alpha = rho_k / p.q, y += alpha p, r -= alpha q, z = M^-1 r, the partial sums of rho_(k+1)
__global__ void __launch_bounds__(kGrThreads)
graph_cg_update_kernel(GraphArgs G, int k)
#if VELO_DEF_GRAPH
{
    __shared__ double buf[kGrThreads];
    if (graph_cg_flags(G.rec) & 1) return;
    const double rho = graph_parts_sum(buf, G.part_rho + (size_t)(k & 1) * G.nb, G.nb);
    const double sigma = graph_parts_sum(buf, G.part_sigma, G.nb);
    if (!(sigma > 0.0) || !isfinite(sigma)) {                          // A is positive definite: a breakdown is an invalid step
        if (blockIdx.x == 0 && threadIdx.x == 0) { G.rec->cg_iters = k; G.rec->cg_rel = 0.0; G.rec->bad = 1; G.rec->cg_done = 1; }
        return;
    }
    const double alpha = rho / sigma;
    const double* p = G.p + (size_t)((k + 1) & 1) * (size_t)G.n_free * 6;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    double rz = 0.0;
    if (i < G.n_free) {
        double r[6], z[6], L[21];
#pragma unroll
        for (int a = 0; a < 21; a++) L[a] = G.chol[(size_t)i * 21 + a];
#pragma unroll
        for (int a = 0; a < 6; a++) {
            G.y[(size_t)i * 6 + a] += alpha * p[(size_t)i * 6 + a];
            r[a] = G.r[(size_t)i * 6 + a] - alpha * G.q[(size_t)i * 6 + a];
            G.r[(size_t)i * 6 + a] = r[a];
        }
        graph_chol_solve(L, r, z);
#pragma unroll
        for (int a = 0; a < 6; a++) { G.zv[(size_t)i * 6 + a] = z[a]; rz += r[a] * z[a]; }
    }
    const double s = graph_block_sum(buf, rz);
    if (threadIdx.x == 0) G.part_rho[(size_t)((k + 1) & 1) * G.nb + blockIdx.x] = s;
}
#else
;
#endif

// ---- the candidate: x_cand = x + c y per free node, the node's share of the model change y.(c g + (c H c) y / 2) and of |c y|^2 --------
// k: the CG iterations enqueued; a solve that ran into that cap records its count and residual here.
__global__ void __launch_bounds__(kGrThreads)
graph_step_kernel(GraphArgs G, int k, int cur)
#if VELO_DEF_GRAPH
{
    __shared__ double buf[kGrThreads];
    if (blockIdx.x == 0 && !(graph_cg_flags(G.rec) & 1)) {
        const double rho = graph_parts_sum(buf, G.part_rho + (size_t)(k & 1) * G.nb, G.nb);
        const double rho0 = graph_parts_sum(buf, G.part_rho0, G.nb);
        if (threadIdx.x == 0) { G.rec->cg_iters = k; G.rec->cg_rel = rho0 > 0.0 ? sqrt(rho / rho0) : 0.0; }
    }
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= G.n_free) return;
    double c[6], y[6], hy[6];
#pragma unroll
    for (int a = 0; a < 6; a++) { c[a] = G.scale[(size_t)i * 6 + a]; y[a] = G.y[(size_t)i * 6 + a]; }
    const double* nd = G.nd + ((size_t)cur * G.n_free + i) * kGrNode;
    graph_diag_mul(nd, c, y, hy);
    const int end = G.inc_start[i + 1];
    for (int m = G.inc_start[i]; m < end; m++) {
        const int code = G.inc[m], e = code >> 1, side = code & 1;
        const int j = G.inc_other[m];
        if (j < 0) continue;
        double v[6];
#pragma unroll
        for (int a = 0; a < 6; a++) v[a] = G.scale[(size_t)j * 6 + a] * G.y[(size_t)j * 6 + a];
        const double* W = G.blk + ((size_t)cur * G.E + e) * kGrBlk + kGrAtB;
#pragma unroll
        for (int a = 0; a < 6; a++) {
            double s = 0.0;
#pragma unroll
            for (int b = 0; b < 6; b++) s += (side ? W[b * 6 + a] : W[a * 6 + b]) * v[b];
            hy[a] += c[a] * s;
        }
    }
    const size_t f6 = (size_t)G.node[i] * 6;
    double model = 0.0, dn2 = 0.0;
#pragma unroll
    for (int a = 0; a < 6; a++) {
        model += y[a] * (nd[21 + a] * c[a] + 0.5 * hy[a]);
        const double d = y[a] * c[a];
        dn2 += d * d;
        G.x[(size_t)(cur ^ 1) * G.x_stride + f6 + a] = G.x[(size_t)cur * G.x_stride + f6 + a] + d;
    }
    G.nterm[(size_t)i * 2] = -model;
    G.nterm[(size_t)i * 2 + 1] = dn2;
}
#else
;
#endif

// ---- one workgroup per scalar of buffer `which`: thread t adds the entries t, t + 256, ... in order, then a fixed tree -------------
__global__ void __launch_bounds__(256)
graph_reduce_kernel(GraphArgs G, int which)
#if VELO_DEF_GRAPH
{
    __shared__ double buf[256];
    const int t = threadIdx.x, idx = blockIdx.x;
    double acc = 0.0;
    if (idx == 0) {
        for (int e = t; e < G.E; e += 256) acc += G.blk[((size_t)which * G.E + e) * kGrBlk + kGrCost];
    } else if (idx < 3) {
        for (int i = t; i < G.n_free; i += 256) acc += G.nterm[(size_t)i * 2 + (idx - 1)];
    } else if (idx == 3) {
        for (int i = t; i < G.n_free; i += 256) {
            const double* x = G.x + (size_t)which * G.x_stride + (size_t)G.node[i] * 6;
            double s = 0.0;
#pragma unroll
            for (int a = 0; a < 6; a++) s += x[a] * x[a];
            acc += s;
        }
    } else {
        for (int i = t; i < G.n_free; i += 256) {
            const double* g = G.nd + ((size_t)which * G.n_free + i) * kGrNode + 21;
#pragma unroll
            for (int a = 0; a < 6; a++) acc = fmax(acc, fabs(g[a]));
        }
    }
    buf[t] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) buf[t] = idx == 4 ? fmax(buf[t], buf[t + s]) : buf[t] + buf[t + s];
        __syncthreads();
    }
    if (t == 0) G.rec->red[idx] = buf[0];
}
#else
;
#endif

// ---- the envelope solver: an exact Cholesky of (c H c + D / mu) in the order of velo_graph_order ------------------------------------
// Row i of the block skyline (i: a position in the order) holds the 6 x 6 row-major blocks of columns first(i) .. i, at
// env + 36 rowptr[i].  Three launches per LM iteration, on one stream:
//     graph_env_fill_kernel    one wave per row, lane l < 36 owns entry l of every block of its row: zero, the damped diagonal block,
//                              then c_i (A^T B)_e c_j for the incident edges whose other end is free and earlier, in the list's order
//     graph_env_factor_kernel  ONE workgroup, in place, right-looking: per step k the Cholesky of the pivot block (thread 0), the
//                              panel L(i,k) = A(i,k) L(k,k)^-T (a thread per block row), the update A(i,j) -= L(i,k) L(j,k)^T (a
//                              thread per block row); a __syncthreads after each; every entry is one fixed-order expression
//     graph_env_solve_kernel   ONE workgroup: b = -c g in the order, forward substitution by rows, back substitution by columns, y
// The panel and the update walk the rows (k, last(k)] and skip a row whose first column lies behind k: the test is uniform per row.
// Nothing waits for another workgroup.  The strict upper triangle of a diagonal block is never read after the fill.
constexpr int kGrEnvFactorThreads = 1024;
constexpr int kGrEnvGroups = kGrEnvFactorThreads / 6;          // groups of 6 threads (a block's rows), one block pair at a time each
constexpr int kGrEnvSolveThreads = 256;
constexpr int kGrEnvChunks = kGrEnvSolveThreads / 6;           // partial sums of a row's forward substitution

__global__ void __launch_bounds__(64)
graph_env_fill_kernel(GraphArgs G, int cur, double mu, int refresh)
#if VELO_DEF_GRAPH
{
    const int i = blockIdx.x, l = threadIdx.x;
    if (i >= G.n_free || l >= 36) return;
    const int a = l / 6, b = l % 6;
    const int node = G.env_perm[i], first = G.env_first[i], w = i - first;
    double* row = G.env + (size_t)G.env_rowptr[i] * 36;
    for (int k = 0; k < w; k++) row[(size_t)k * 36 + l] = 0.0;
    const double* nd = G.nd + ((size_t)cur * G.n_free + node) * kGrNode;
    const double ca = G.scale[(size_t)node * 6 + a], cb = G.scale[(size_t)node * 6 + b];
    double d = nd[upper6(a < b ? a : b, a < b ? b : a)] * ca * cb;
    if (a == b) {                                                      // D as the CG's M_i has it: clipped, refreshed on acceptance
        double dg = G.diag[(size_t)node * 6 + a];
        if (refresh) { dg = fmin(fmax(d, G.lm.min_diag), G.lm.max_diag); G.diag[(size_t)node * 6 + a] = dg; }
        d += dg / mu;
    }
    row[(size_t)w * 36 + l] = d;
    const int end = G.inc_start[node + 1];
    for (int m = G.inc_start[node]; m < end; m++) {
        const int j = G.inc_other[m];
        if (j < 0) continue;                                           // the other end is a constant
        const int pj = G.env_pos[j];
        if (pj >= i) continue;                                         // the later end's row holds this block
        const int code = G.inc[m];
        const double* W = G.blk + ((size_t)cur * G.E + (code >> 1)) * kGrBlk + kGrAtB;
        const double v = (code & 1) ? W[b * 6 + a] : W[a * 6 + b];    // transposed on the `to` side
        row[(size_t)(pj - first) * 36 + l] += (ca * v) * G.scale[(size_t)j * 6 + b];
    }
}
#else
;
#endif

// graph_chol6 with one division per column, not one per entry: the pivot's Cholesky is a single thread's chain of dependent fp64
// operations in every elimination step, and a division is some forty of them.  inv: 1 / the diagonal of L.
__device__ __forceinline__ bool graph_env_chol6(double M[36], double inv[6]) {
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double dj = M[j * 6 + j];
#pragma unroll
        for (int k = 0; k < j; k++) dj -= M[j * 6 + k] * M[j * 6 + k];
        if (!(dj > 0.0) || !isfinite(dj)) { ok = false; dj = 1.0; }
        const double l = sqrt(dj);
        M[j * 6 + j] = l;
        inv[j] = 1.0 / l;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double s = M[i * 6 + j];
#pragma unroll
            for (int k = 0; k < j; k++) s -= M[i * 6 + k] * M[j * 6 + k];
            M[i * 6 + j] = s * inv[j];
        }
    }
    return ok;
}

__global__ void __launch_bounds__(kGrEnvFactorThreads)
graph_env_factor_kernel(GraphArgs G)
#if VELO_DEF_GRAPH
{
    __shared__ double piv[36];                                         // L(k,k), lower triangle
    __shared__ double pinv[6];                                         // 1 / its diagonal
    __shared__ int bad_s;
    const int t = threadIdx.x, n = G.n_free;
    const int ea = t % 6, g = t / 6;
    if (t == 0) { bad_s = 0; G.rec->cg_done = 1; }                     // no CG ran: the record keeps cg_iters = 0, cg_rel = 0
    for (int k = 0; k < n; k++) {
        const int fk = G.env_first[k];
        if (t == 0) {
            double* D = G.env + ((size_t)G.env_rowptr[k] + (size_t)(k - fk)) * 36;
            double M[36];
#pragma unroll
            for (int x = 0; x < 36; x++) M[x] = D[x];
            double inv[6];
            if (!graph_env_chol6(M, inv)) bad_s = 1;
#pragma unroll
            for (int r = 0; r < 6; r++) {
#pragma unroll
                for (int c = 0; c <= r; c++) { D[r * 6 + c] = M[r * 6 + c]; piv[r * 6 + c] = M[r * 6 + c]; }
                pinv[r] = inv[r];
            }
        }
        __syncthreads();
        if (bad_s) {                                                   // a pivot that is not positive and finite: an invalid step
            if (t == 0) G.rec->bad = 1;
            return;
        }
        const int m = G.env_last[k] - k;                               // the rows k + 1 .. k + m can hold a block in column k
        for (int u = t; u < m * 6; u += kGrEnvFactorThreads) {         // the panel: row r of L(i,k) = A(i,k) L(k,k)^-T
            const int i = k + 1 + u / 6, r = u % 6, fi = G.env_first[i];
            if (fi > k) continue;
            double* A = G.env + ((size_t)G.env_rowptr[i] + (size_t)(k - fi)) * 36 + r * 6;
            double x[6];
#pragma unroll
            for (int c = 0; c < 6; c++) {
                double s = A[c];
#pragma unroll
                for (int q = 0; q < c; q++) s -= x[q] * piv[c * 6 + q];
                x[c] = s * pinv[c];
            }
#pragma unroll
            for (int c = 0; c < 6; c++) A[c] = x[c];
        }
        __syncthreads();
        if (g < kGrEnvGroups) {                                        // the update: row ea of A(i,j) -= L(i,k) L(j,k)^T, i >= j > k
            int ii = 0, jj = g;                                        // pair number p = ii (ii + 1) / 2 + jj, p = g, g + groups, ...
            for (;;) {
                while (jj > ii) { jj -= ii + 1; ii++; }
                if (ii >= m) break;
                const int i = k + 1 + ii, j = k + 1 + jj, fi = G.env_first[i], fj = G.env_first[j];
                if (fi <= k && fj <= k) {                              // then first(i) <= k < j: (i,j) lies inside the envelope
                    const double* Li = G.env + ((size_t)G.env_rowptr[i] + (size_t)(k - fi)) * 36 + ea * 6;
                    const double* Lj = G.env + ((size_t)G.env_rowptr[j] + (size_t)(k - fj)) * 36;
                    double* A = G.env + ((size_t)G.env_rowptr[i] + (size_t)(j - fi)) * 36 + ea * 6;
                    double li[6], lj[36], s[6];                        // every load of the pair is requested before its first store
#pragma unroll
                    for (int c = 0; c < 6; c++) { li[c] = Li[c]; s[c] = A[c]; }
#pragma unroll
                    for (int x = 0; x < 36; x++) lj[x] = Lj[x];
#pragma unroll
                    for (int b = 0; b < 6; b++) {
#pragma unroll
                        for (int c = 0; c < 6; c++) s[b] -= li[c] * lj[b * 6 + c];
                    }
#pragma unroll
                    for (int b = 0; b < 6; b++) A[b] = s[b];
                }
                jj += kGrEnvGroups;
            }
        }
        __syncthreads();
    }
}
#else
;
#endif

// graph_env_factor_kernel for an APPEND to a retained factor (velo_graph_retain): the rows < row_begin of the skyline hold their final L,
// the rows >= row_begin hold H~ fresh from the fill.  It starts at step k0 = min first(i) over i >= row_begin (the host's); for
// k < row_begin the pivot is read back from the stored diagonal block (pinv = 1.0 / l, as graph_env_chol6 forms it) and the panel and
// the update touch the block rows i >= row_begin alone, in all their columns j in (k, i]; from k = row_begin on it is the full step.
// Every entry of the rows >= row_begin so receives exactly the operations of a full factorisation in the same order, in the same
// sequence: an entry is written by one thread per step, the steps are separated by barriers, and which thread it is does not enter the
// expression.  The row test guards work, never a barrier: every __syncthreads is reached by every thread of the workgroup (the return
// on a bad pivot is taken by all of them: bad_s is read behind the barrier).
// Its text repeats graph_env_factor_kernel's, which stays as it is: as two instances of one template body the full factorisation's
// instance came out with other instructions than before, and that kernel is what every solve is measured on.
__global__ void __launch_bounds__(kGrEnvFactorThreads)
graph_env_factor_rows_kernel(GraphArgs G, int row_begin, int k0)
#if VELO_DEF_GRAPH
{
    __shared__ double piv[36];                                         // L(k,k), lower triangle
    __shared__ double pinv[6];                                         // 1 / its diagonal
    __shared__ int bad_s;
    const int t = threadIdx.x, n = G.n_free;
    const int ea = t % 6, g = t / 6;
    if (t == 0) { bad_s = 0; G.rec->cg_done = 1; }                     // no CG ran: the record keeps cg_iters = 0, cg_rel = 0
    for (int k = k0; k < n; k++) {
        const int fk = G.env_first[k];
        if (t == 0) {
            double* D = G.env + ((size_t)G.env_rowptr[k] + (size_t)(k - fk)) * 36;
            if (k < row_begin) {                                       // a row that keeps its factor: L(k,k) as it was stored
#pragma unroll
                for (int r = 0; r < 6; r++) {
#pragma unroll
                    for (int c = 0; c <= r; c++) piv[r * 6 + c] = D[r * 6 + c];
                    pinv[r] = 1.0 / D[r * 6 + r];
                }
            } else {
                double M[36];
#pragma unroll
                for (int x = 0; x < 36; x++) M[x] = D[x];
                double inv[6];
                if (!graph_env_chol6(M, inv)) bad_s = 1;
#pragma unroll
                for (int r = 0; r < 6; r++) {
#pragma unroll
                    for (int c = 0; c <= r; c++) { D[r * 6 + c] = M[r * 6 + c]; piv[r * 6 + c] = M[r * 6 + c]; }
                    pinv[r] = inv[r];
                }
            }
        }
        __syncthreads();
        if (bad_s) {                                                   // a pivot that is not positive and finite: an invalid step
            if (t == 0) G.rec->bad = 1;
            return;
        }
        const int m = G.env_last[k] - k;                               // the rows k + 1 .. k + m can hold a block in column k
        const int skip = row_begin > k + 1 ? row_begin - k - 1 : 0;    // of them the first `skip` keep their factor
        for (int u = skip * 6 + t; u < m * 6; u += kGrEnvFactorThreads) {      // the panel: row r of L(i,k) = A(i,k) L(k,k)^-T
            const int i = k + 1 + u / 6, r = u % 6, fi = G.env_first[i];
            if (fi > k) continue;
            double* A = G.env + ((size_t)G.env_rowptr[i] + (size_t)(k - fi)) * 36 + r * 6;
            double x[6];
#pragma unroll
            for (int c = 0; c < 6; c++) {
                double s = A[c];
#pragma unroll
                for (int q = 0; q < c; q++) s -= x[q] * piv[c * 6 + q];
                x[c] = s * pinv[c];
            }
#pragma unroll
            for (int c = 0; c < 6; c++) A[c] = x[c];
        }
        __syncthreads();
        if (g < kGrEnvGroups) {                                        // the update: row ea of A(i,j) -= L(i,k) L(j,k)^T, i >= j > k
            int ii = skip, jj = g;                                     // pair number p = ii (ii + 1) / 2 + jj, p = g, g + groups, ... (from row `skip` on)
            for (;;) {
                while (jj > ii) { jj -= ii + 1; ii++; }
                if (ii >= m) break;
                const int i = k + 1 + ii, j = k + 1 + jj, fi = G.env_first[i], fj = G.env_first[j];
                if (fi <= k && fj <= k) {                              // then first(i) <= k < j: (i,j) lies inside the envelope
                    const double* Li = G.env + ((size_t)G.env_rowptr[i] + (size_t)(k - fi)) * 36 + ea * 6;
                    const double* Lj = G.env + ((size_t)G.env_rowptr[j] + (size_t)(k - fj)) * 36;
                    double* A = G.env + ((size_t)G.env_rowptr[i] + (size_t)(j - fi)) * 36 + ea * 6;
                    double li[6], lj[36], s[6];                        // every load of the pair is requested before its first store
#pragma unroll
                    for (int c = 0; c < 6; c++) { li[c] = Li[c]; s[c] = A[c]; }
#pragma unroll
                    for (int x = 0; x < 36; x++) lj[x] = Lj[x];
#pragma unroll
                    for (int b = 0; b < 6; b++) {
#pragma unroll
                        for (int c = 0; c < 6; c++) s[b] -= li[c] * lj[b * 6 + c];
                    }
#pragma unroll
                    for (int b = 0; b < 6; b++) A[b] = s[b];
                }
                jj += kGrEnvGroups;
            }
        }
        __syncthreads();
    }
}
#else
;
#endif

__global__ void __launch_bounds__(kGrEnvSolveThreads)
graph_env_solve_kernel(GraphArgs G, int cur)
#if VELO_DEF_GRAPH
{
    __shared__ double part[kGrEnvChunks * 6];
    __shared__ double xs[6];
    if (G.rec->bad != 0) return;                                       // (the same word for every thread: the factorisation's launch wrote it)
    const int t = threadIdx.x, n = G.n_free;
    const int a = t % 6, ch = t / 6;
    double* v = G.r;                                                   // [n_free][6] by position: b, then L^-1 b, then the solution
    for (int u = t; u < n * 6; u += kGrEnvSolveThreads) {
        const int node = G.env_perm[u / 6], c = u % 6;
        v[u] = -(G.nd[((size_t)cur * n + node) * kGrNode + 21 + c] * G.scale[(size_t)node * 6 + c]);
    }
    __syncthreads();
    for (int i = 0; i < n; i++) {                                      // forward, by rows: x_i = L(i,i)^-1 (b_i - sum_j L(i,j) x_j)
        const int fi = G.env_first[i], w = i - fi;
        const double* row = G.env + (size_t)G.env_rowptr[i] * 36;
        if (ch < kGrEnvChunks) {
            double s = 0.0;
            for (int j = ch; j < w; j += kGrEnvChunks) {
                const double* L = row + (size_t)j * 36 + a * 6;
                const double* x = v + (size_t)(fi + j) * 6;
#pragma unroll
                for (int c = 0; c < 6; c++) s += L[c] * x[c];
            }
            part[ch * 6 + a] = s;
        }
        __syncthreads();
        if (t < 64) {                                                  // the first wave: lane a sums the chunks in order, every lane then
            double s = 0.0;                                            // solves the 6 x 6 triangle and lane a keeps component a
            if (t < 6) {
                s = v[(size_t)i * 6 + t];
                const int nc = w < kGrEnvChunks ? w : kGrEnvChunks;
                for (int c = 0; c < nc; c++) s -= part[c * 6 + t];
            }
            double x[6];
#pragma unroll
            for (int c = 0; c < 6; c++) x[c] = __shfl(s, c);
            if (t < 6) {
                const double* D = row + (size_t)w * 36;
#pragma unroll
                for (int r = 0; r < 6; r++) {
                    double q = x[r];
#pragma unroll
                    for (int c = 0; c < r; c++) q -= D[r * 6 + c] * x[c];
                    x[r] = q / D[r * 6 + r];
                }
                double mine = x[0];
#pragma unroll
                for (int c = 1; c < 6; c++) if (t == c) mine = x[c];
                v[(size_t)i * 6 + t] = mine;
            }
        }
        __syncthreads();
    }
    for (int i = n - 1; i >= 0; i--) {                                 // back, by columns: x_i = L(i,i)^-T b_i, then b_j -= L(i,j)^T x_i
        const int fi = G.env_first[i], w = i - fi;
        const double* row = G.env + (size_t)G.env_rowptr[i] * 36;
        if (t < 64) {
            const double s = t < 6 ? v[(size_t)i * 6 + t] : 0.0;
            double x[6];
#pragma unroll
            for (int c = 0; c < 6; c++) x[c] = __shfl(s, c);
            if (t < 6) {
                const double* D = row + (size_t)w * 36;
#pragma unroll
                for (int r = 5; r >= 0; r--) {
                    double q = x[r];
#pragma unroll
                    for (int c = r + 1; c < 6; c++) q -= D[c * 6 + r] * x[c];
                    x[r] = q / D[r * 6 + r];
                }
                double mine = x[0];
#pragma unroll
                for (int c = 1; c < 6; c++) if (t == c) mine = x[c];
                v[(size_t)i * 6 + t] = mine;
                xs[t] = mine;
            }
        }
        __syncthreads();
        for (int u = t; u < w * 6; u += kGrEnvSolveThreads) {
            const int j = u / 6, c = u % 6;
            const double* L = row + (size_t)j * 36;
            double s = v[(size_t)(fi + j) * 6 + c];
#pragma unroll
            for (int r = 0; r < 6; r++) s -= L[r * 6 + c] * xs[r];
            v[(size_t)(fi + j) * 6 + c] = s;
        }
        __syncthreads();
    }
    for (int u = t; u < n * 6; u += kGrEnvSolveThreads)               // the step y, by free index, where graph_step_kernel reads it
        G.y[(size_t)G.env_perm[u / 6] * 6 + u % 6] = v[u];
}
#else
;
#endif

// ---- covariances of the poses: blocks of (J^T J)^-1 from the envelope factor (velo_graph_covariance) ---------------------------------
// H~ = c H c is the UNDAMPED Jacobi-scaled normal matrix (c = G.scale, which graph_assemble_kernel sets from this call's H in every
// graph_begin: no history of G.diag in it), L its envelope Cholesky factor, Z = H~^-1.  Sigma_ab = c_a Z_ab c_b.  On one stream:
//     graph_env_fill_undamped_kernel  graph_env_fill_kernel's fill of buffer 0 without the D / mu term; G.diag is not touched
//     graph_env_factor_kernel         as above; a pivot that is not positive sets the record's `bad` and ends what follows
//     graph_env_selinv_kernel         ONE workgroup: the entries of Z inside the envelope (the selected inverse), lower triangle, into a
//                                     second skyline with the same rowptr, by the Takahashi recursion.  Columns j = n - 1 .. 0 over
//                                     S_j = { i in (j, last(j)] : first(i) <= j }.  The envelope is closed under it: for i, k in S_j, k > i,
//                                     first(k) <= j < i, so (k, i) is stored.  Per column: thread 0 inverts L(j,j) into LDS; the panel
//                                     Z(i,j) = -(sum_{k in S_j} Z(i,k) L(k,j)) L(j,j)^-1, a thread per block row, Z(i,k) = Z(k,i)^T for k > i;
//                                     the diagonal Z(j,j) = (L(j,j)^-T - sum_k Z(k,j)^T L(k,j)) L(j,j)^-1, a thread per entry, the lower
//                                     triangle computed and mirrored, so the block is symmetric to the bit.  A __syncthreads after each.
//                                     A row's sum over k is dealt to as many threads as the workgroup has for it (chunk c takes k = j + 1 + c,
//                                     j + 1 + c + chunks, ..., ascending, into LDS) and the row's thread adds the chunks in order; likewise
//                                     the 36 entries of the diagonal's sum, 28 chunks each.  Where a column reaches more than 85 rows a thread
//                                     carries its row's whole sum.  The split depends on the column alone, so every entry is one fixed-order expression;
//                                     no atomics.  The panel reads columns > j of Z only and writes column j only.
//     graph_env_column_kernel         one workgroup per pair OUTSIDE the envelope, independent of one another: with positions hi > lo the
//                                     6 columns of Z that belong to lo, as far as row hi: forward substitution of E_lo from row lo on, back
//                                     substitution from row n - 1 down to hi.  The work vector ([n][36], a 6 x 6 per row) is the
//                                     workgroup's slice of a scratch buffer.  Two components of the free graph occupy disjoint position
//                                     ranges, so across them every term of the forward sum is zero and the block is an exact zero.
//     graph_cov_gather_kernel         one workgroup per pair: Z or Z^T from the skyline or from a column's row hi, times c_a c_b, into
//                                     the output staging behind the record; zeros for a pair that names a constant.
// The rows of a 6 x 6 are short dependent fp64 chains; as in the factor kernel a thread owns a block row and requests its loads together.
constexpr int kGrEnvSelinvThreads = 1024;
constexpr int kGrEnvSelinvChunks = kGrEnvSelinvThreads / 36;   // partial sums of an entry of the diagonal block
constexpr int kGrEnvColumnThreads = 256;
constexpr int kGrEnvColumnChunks = kGrEnvColumnThreads / 36;   // partial sums of a row's forward substitution

struct GraphCov {
    double* zenv;                                // [blocks][36]: Z inside the envelope, lower triangle, rows as in G.env
    double* work;                                // [n_out][n_free][36]: the column kernel's work vectors
    const int* pair;                             // [n_pairs][3]: free index of a, of b (-1: a constant), column slot (-1: inside the envelope)
    double* out;                                 // [n_pairs][36]
    int n_pairs;
};

__global__ void __launch_bounds__(64)
graph_env_fill_undamped_kernel(GraphArgs G)
#if VELO_DEF_GRAPH
{
    const int i = blockIdx.x, l = threadIdx.x;
    if (i >= G.n_free || l >= 36) return;
    const int a = l / 6, b = l % 6;
    const int node = G.env_perm[i], first = G.env_first[i], w = i - first;
    double* row = G.env + (size_t)G.env_rowptr[i] * 36;
    for (int k = 0; k < w; k++) row[(size_t)k * 36 + l] = 0.0;
    const double* nd = G.nd + (size_t)node * kGrNode;                  // the stored state is buffer 0
    const double ca = G.scale[(size_t)node * 6 + a], cb = G.scale[(size_t)node * 6 + b];
    row[(size_t)w * 36 + l] = nd[upper6(a < b ? a : b, a < b ? b : a)] * ca * cb;
    const int end = G.inc_start[node + 1];
    for (int m = G.inc_start[node]; m < end; m++) {
        const int j = G.inc_other[m];
        if (j < 0) continue;                                           // the other end is a constant
        const int pj = G.env_pos[j];
        if (pj >= i) continue;                                         // the later end's row holds this block
        const int code = G.inc[m];
        const double* W = G.blk + (size_t)(code >> 1) * kGrBlk + kGrAtB;
        const double v = (code & 1) ? W[b * 6 + a] : W[a * 6 + b];    // transposed on the `to` side
        row[(size_t)(pj - first) * 36 + l] += (ca * v) * G.scale[(size_t)j * 6 + b];
    }
}
#else
;
#endif

// graph_env_fill_undamped_kernel for the rows row_begin .. n_free - 1 alone (workgroup w: row row_begin + w): what an append to a
// retained factor refills; the rows before keep their L
__global__ void __launch_bounds__(64)
graph_env_fill_undamped_rows_kernel(GraphArgs G, int row_begin)
#if VELO_DEF_GRAPH
{
    const int i = row_begin + (int)blockIdx.x, l = threadIdx.x;
    if (i >= G.n_free || l >= 36) return;
    const int a = l / 6, b = l % 6;
    const int node = G.env_perm[i], first = G.env_first[i], w = i - first;
    double* row = G.env + (size_t)G.env_rowptr[i] * 36;
    for (int k = 0; k < w; k++) row[(size_t)k * 36 + l] = 0.0;
    const double* nd = G.nd + (size_t)node * kGrNode;                  // the stored state is buffer 0
    const double ca = G.scale[(size_t)node * 6 + a], cb = G.scale[(size_t)node * 6 + b];
    row[(size_t)w * 36 + l] = nd[upper6(a < b ? a : b, a < b ? b : a)] * ca * cb;
    const int end = G.inc_start[node + 1];
    for (int m = G.inc_start[node]; m < end; m++) {
        const int j = G.inc_other[m];
        if (j < 0) continue;                                           // the other end is a constant
        const int pj = G.env_pos[j];
        if (pj >= i) continue;                                         // the later end's row holds this block
        const int code = G.inc[m];
        const double* W = G.blk + (size_t)(code >> 1) * kGrBlk + kGrAtB;
        const double v = (code & 1) ? W[b * 6 + a] : W[a * 6 + b];    // transposed on the `to` side
        row[(size_t)(pj - first) * 36 + l] += (ca * v) * G.scale[(size_t)j * 6 + b];
    }
}
#else
;
#endif

// X = L^-1 for the lower triangle of a 6 x 6 block, column by column; the strict upper triangle of X is zero
// (L: packed, row-major; X: 36 doubles in LDS, written and read back by the one calling thread)
__device__ __forceinline__ void graph_env_inv6(const double L[21], double* X) {
    double d[6];
#pragma unroll
    for (int i = 0; i < 6; i++) d[i] = 1.0 / L[graph_lower6(i, i)];
#pragma unroll
    for (int c = 0; c < 6; c++) {
        double x[6];                                                   // column c
#pragma unroll
        for (int i = 0; i < 6; i++) {
            double s = 0.0;
#pragma unroll
            for (int q = c; q < i; q++) s -= L[graph_lower6(i, q)] * x[q];
            x[i] = i < c ? 0.0 : (i == c ? d[i] : s * d[i]);
            X[i * 6 + c] = x[i];
        }
    }
}

// the part k = k0, k0 + step, ... <= j + m of row r of sum_{k in S_j} Z(i,k) L(k,j), k ascending
__device__ __forceinline__ void graph_env_selinv_row(const GraphArgs& G, const GraphCov& V, int i, int r, int fi, int j, int m, int k0, int step, double s[6]) {
    const size_t zi = (size_t)G.env_rowptr[i];
    for (int k = k0; k <= j + m; k += step) {
        const int fk = G.env_first[k];
        if (fk > j) continue;
        const double* Lk = G.env + ((size_t)G.env_rowptr[k] + (size_t)(j - fk)) * 36;
        double z[6];
        if (k <= i) {
            const double* Z = V.zenv + (zi + (size_t)(k - fi)) * 36 + r * 6;
#pragma unroll
            for (int c = 0; c < 6; c++) z[c] = Z[c];
        } else {                                                       // first(k) <= j < i: (k,i) is stored, read transposed
            const double* Z = V.zenv + ((size_t)G.env_rowptr[k] + (size_t)(i - fk)) * 36 + r;
#pragma unroll
            for (int c = 0; c < 6; c++) z[c] = Z[c * 6];
        }
#pragma unroll
        for (int c = 0; c < 6; c++) {                                  // a row of L(k,j) at a time: 36 doubles of it in registers spill
            double lk[6];
#pragma unroll
            for (int b = 0; b < 6; b++) lk[b] = Lk[c * 6 + b];
#pragma unroll
            for (int b = 0; b < 6; b++) s[b] += z[c] * lk[b];
        }
    }
}

__global__ void __launch_bounds__(kGrEnvSelinvThreads)
graph_env_selinv_kernel(GraphArgs G, GraphCov V)
#if VELO_DEF_GRAPH
{
    __shared__ double linv[36];                                        // L(j,j)^-1, the upper triangle zero
    __shared__ double part[kGrEnvSelinvThreads * 6];                   // chunk sums: of the panel's rows, then of the diagonal's entries
    if (G.rec->bad != 0) return;                                       // (the same word for every thread: the factorisation's launch wrote it)
    const int t = threadIdx.x, n = G.n_free;
    for (int j = n - 1; j >= 0; j--) {
        const int fj = G.env_first[j];
        const int m = G.env_last[j] - j;                               // the rows j + 1 .. j + m can hold a block in column j
        const int rows = m * 6;
        // a panel row's sum over k is dealt to `chunks` threads (k = j + 1 + c, j + 1 + c + chunks, ...) when the workgroup has them
        int chunks = rows > 0 ? kGrEnvSelinvThreads / rows : 0;
        if (chunks > m) chunks = m;
        if (t == kGrEnvSelinvThreads - 1) {                            // (the thread least likely to hold a chunk)
            double Lb[21];
            const double* D = G.env + ((size_t)G.env_rowptr[j] + (size_t)(j - fj)) * 36;
#pragma unroll
            for (int r = 0; r < 6; r++) {
#pragma unroll
                for (int c = 0; c <= r; c++) Lb[graph_lower6(r, c)] = D[r * 6 + c];
            }
            graph_env_inv6(Lb, linv);
        }
        if (chunks >= 2 && t < rows * chunks) {
            const int u = t % rows, ch = t / rows;
            const int i = j + 1 + u / 6, r = u % 6, fi = G.env_first[i];
            double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (fi <= j) graph_env_selinv_row(G, V, i, r, fi, j, m, j + 1 + ch, chunks, s);
#pragma unroll
            for (int b = 0; b < 6; b++) part[(size_t)t * 6 + b] = s[b];
        }
        __syncthreads();
        for (int u = t; u < rows; u += kGrEnvSelinvThreads) {          // the panel: row r of Z(i,j) = -(the sum) L(j,j)^-1
            const int i = j + 1 + u / 6, r = u % 6, fi = G.env_first[i];
            if (fi > j) continue;
            double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
            if (chunks >= 2) {                                         // (then rows <= 512: one trip, u == t)
                for (int ch = 0; ch < chunks; ch++) {
#pragma unroll
                    for (int b = 0; b < 6; b++) s[b] += part[((size_t)ch * rows + u) * 6 + b];
                }
            } else graph_env_selinv_row(G, V, i, r, fi, j, m, j + 1, 1, s);
            double* out = V.zenv + ((size_t)G.env_rowptr[i] + (size_t)(j - fi)) * 36 + r * 6;
#pragma unroll
            for (int c = 0; c < 6; c++) {
                double v = 0.0;
#pragma unroll
                for (int b = c; b < 6; b++) v -= s[b] * linv[b * 6 + c];
                out[c] = v;
            }
        }
        __syncthreads();
        const int dch = m < kGrEnvSelinvChunks ? m : kGrEnvSelinvChunks;
        if (t < 36 * dch) {                                            // entry (r, c) of sum_k Z(k,j)^T L(k,j): a chunk of the k
            const int e = t % 36, ch = t / 36, r = e / 6, c = e % 6;
            double s = 0.0;
            for (int k = j + 1 + ch; k <= j + m; k += dch) {
                const int fk = G.env_first[k];
                if (fk > j) continue;
                const size_t o = ((size_t)G.env_rowptr[k] + (size_t)(j - fk)) * 36;
                const double* Lk = G.env + o;
                const double* Zk = V.zenv + o;
#pragma unroll
                for (int q = 0; q < 6; q++) s += Zk[q * 6 + r] * Lk[q * 6 + c];
            }
            part[t] = s;
        }
        __syncthreads();
        if (t < 36) {                                                  // Z(j,j) = (L(j,j)^-T - the sum) L(j,j)^-1: the lower triangle, mirrored
            const int r = t / 6, c = t % 6;
            if (c <= r) {
                double v = 0.0;
#pragma unroll
                for (int b = 0; b < 6; b++) {
                    double w = linv[b * 6 + r];
                    for (int ch = 0; ch < dch; ch++) w -= part[ch * 36 + r * 6 + b];
                    v += w * linv[b * 6 + c];
                }
                double* Zj = V.zenv + ((size_t)G.env_rowptr[j] + (size_t)(j - fj)) * 36;
                Zj[r * 6 + c] = v;
                Zj[c * 6 + r] = v;
            }
        }
        __syncthreads();
    }
}
#else
;
#endif

// The 6 columns of Z that belong to position lo, rows hi .. n - 1, into the work vector v (row i: the 6 x 6 of the 6 right-hand sides): the
// text graph_env_column_kernel (one pair: as far as row hi) and graph_env_column_full_kernel (hi = 0: the whole block column) share.  The
// back substitution reads the rows [hi, lo) as zeros, which the full kernel writes there first.  ints: the pairs ([n_pairs][3], as
// GraphCov::pair), or for the full kernel the position of every slot's column.
template <bool kFull>
__device__ __forceinline__ void graph_env_column_body(const GraphArgs& G, double* work, const int* ints, int n_pairs) {
    __shared__ double part[kGrEnvColumnChunks * 36];
    __shared__ double xs[36];
    __shared__ int pair_s[2];
    if (G.rec->bad != 0) return;
    const int t = threadIdx.x, n = G.n_free;
    if (t == 0) {                                                      // the pair that holds this workgroup's slot
        int pa = 0, pb = 0;
        for (int p = 0; !kFull && p < n_pairs; p++)
            if (ints[p * 3 + 2] == (int)blockIdx.x) { pa = G.env_pos[ints[p * 3]]; pb = G.env_pos[ints[p * 3 + 1]]; break; }
        pair_s[0] = kFull ? 0 : pa > pb ? pa : pb;
        pair_s[1] = kFull ? ints[blockIdx.x] : pa > pb ? pb : pa;
    }
    __syncthreads();
    const int hi = pair_s[0], lo = pair_s[1];
    double* v = work + (size_t)blockIdx.x * (size_t)n * 36;            // row i: the 6 x 6 of the 6 right-hand sides
    if (kFull) {
        for (int u = t; u < lo * 36; u += kGrEnvColumnThreads) v[u] = 0.0;
        __syncthreads();
    }
    const int e = t % 36, ch = t / 36, er = e / 6, ec = e % 6;
    for (int i = lo; i < n; i++) {                                     // forward, by rows: Y_i = L(i,i)^-1 (E_i - sum_j L(i,j) Y_j), Y_j = 0 for j < lo
        const int fi = G.env_first[i];
        const int j0 = fi > lo ? fi : lo;
        const double* row = G.env + (size_t)G.env_rowptr[i] * 36;
        if (ch < kGrEnvColumnChunks) {
            double s = 0.0;
            for (int j = j0 + ch; j < i; j += kGrEnvColumnChunks) {
                const double* L = row + (size_t)(j - fi) * 36 + er * 6;
                const double* y = v + (size_t)j * 36 + ec;
#pragma unroll
                for (int q = 0; q < 6; q++) s += L[q] * y[q * 6];
            }
            part[ch * 36 + e] = s;
        }
        __syncthreads();
        if (t < 6) {                                                   // thread c: column c of the block, the chunks in order, then the triangle
            const double* D = row + (size_t)(i - fi) * 36;
            const int w = i - j0;
            const int nc = w < kGrEnvColumnChunks ? w : kGrEnvColumnChunks;
            double x[6];
#pragma unroll
            for (int r = 0; r < 6; r++) {
                double q = (i == lo && r == t) ? 1.0 : 0.0;
                for (int c = 0; c < nc; c++) q -= part[c * 36 + r * 6 + t];
#pragma unroll
                for (int c = 0; c < r; c++) q -= D[r * 6 + c] * x[c];
                x[r] = q / D[r * 6 + r];
            }
#pragma unroll
            for (int r = 0; r < 6; r++) v[(size_t)i * 36 + r * 6 + t] = x[r];
        }
        __syncthreads();
    }
    for (int i = n - 1; i >= hi; i--) {                                // back, by columns: X_i = L(i,i)^-T Y_i, then Y_j -= L(i,j)^T X_i for hi <= j < i
        const int fi = G.env_first[i];
        const int j0 = fi > hi ? fi : hi;
        const double* row = G.env + (size_t)G.env_rowptr[i] * 36;
        if (t < 6) {
            const double* D = row + (size_t)(i - fi) * 36;
            double x[6];
#pragma unroll
            for (int r = 5; r >= 0; r--) {
                double q = v[(size_t)i * 36 + r * 6 + t];
#pragma unroll
                for (int c = r + 1; c < 6; c++) q -= D[c * 6 + r] * x[c];
                x[r] = q / D[r * 6 + r];
            }
#pragma unroll
            for (int r = 0; r < 6; r++) { v[(size_t)i * 36 + r * 6 + t] = x[r]; xs[r * 6 + t] = x[r]; }
        }
        __syncthreads();
        for (int u = t; u < (i - j0) * 36; u += kGrEnvColumnThreads) {
            const int j = j0 + u / 36, r = (u % 36) / 6, c = u % 6;
            const double* L = row + (size_t)(j - fi) * 36;
            double s = v[(size_t)j * 36 + r * 6 + c];
#pragma unroll
            for (int q = 0; q < 6; q++) s -= L[q * 6 + r] * xs[q * 6 + c];
            v[(size_t)j * 36 + r * 6 + c] = s;
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kGrEnvColumnThreads)
graph_env_column_kernel(GraphArgs G, GraphCov V)
#if VELO_DEF_GRAPH
{
    graph_env_column_body<false>(G, V.work, V.pair, V.n_pairs);
}
#else
;
#endif

__global__ void __launch_bounds__(64)
graph_cov_gather_kernel(GraphArgs G, GraphCov V)
#if VELO_DEF_GRAPH
{
    const int p = blockIdx.x, l = threadIdx.x;
    if (p >= V.n_pairs || l >= 36) return;
    const int r = l / 6, c = l % 6;
    const int ia = V.pair[p * 3], ib = V.pair[p * 3 + 1], slot = V.pair[p * 3 + 2];
    double out = 0.0;                                                  // a constant has no uncertainty
    if (ia >= 0 && ib >= 0 && G.rec->bad == 0) {
        const int pa = G.env_pos[ia], pb = G.env_pos[ib];
        const int hi = pa > pb ? pa : pb, lo = pa > pb ? pb : pa;
        const double* B = slot >= 0 ? V.work + ((size_t)slot * (size_t)G.n_free + (size_t)hi) * 36
                                    : V.zenv + ((size_t)G.env_rowptr[hi] + (size_t)(lo - G.env_first[hi])) * 36;
        const double z = pa >= pb ? B[r * 6 + c] : B[c * 6 + r];      // the stored block is Z(hi, lo)
        out = z * (G.scale[(size_t)ia * 6 + r] * G.scale[(size_t)ib * 6 + c]);
    }
    V.out[(size_t)p * 36 + l] = out;
}
#else
;
#endif

// ---- the covariance of a relative pose in an edge's tangent space (velo_graph_edge_gate, velo_graph_loop_candidates) -------------------
// For a pair (a, b) and a measurement Z the unweighted edge residual r = pose_vec(Z^-1 T_a^-1 T_b) has the Jacobians A, B of
// graph_edge_terms_at, and to first order Cov(r) = Sigma_rel = A S_aa A^T + A S_ab B^T + B S_ba A^T + B S_bb B^T with the blocks S of
// velo_graph_covariance -- which, unlike them, does not depend on the frame that is fixed.  Behind the factor and the selected inverse
// of velo_graph_covariance, on the same stream:
//     graph_env_column_full_kernel   one workgroup per DISTINCT frame that a pair outside the envelope needs a column of: the whole block
//                                    column of Z at its position q, rows 0 .. n - 1 (graph_env_column_body with hi = 0, the rows above q
//                                    cleared first), so that every pair that shares the frame reads its cross block off one solve
//     graph_relcov_kernel            one workgroup per pair: thread 0 forms rel = pose_vec(T_a^-1 T_b), takes Z (the caller's, or rel itself),
//                                    r, A, B and, where the pair has an information W = L L^T, L^-1; the three blocks are gathered with the
//                                    Jacobi scales as graph_cov_gather_kernel gathers them (zeros for a constant); T1 = S_aa A^T + S_ab B^T and
//                                    T2 = S_ba A^T + S_bb B^T, a thread per entry; then S = A T1 + B T2 + W^-1, a thread per entry of the lower
//                                    triangle, mirrored, so S is symmetric to the bit; thread 0 factors S and writes chi2 = r^T S^-1 r, or -1
//                                    where a pivot is not positive and finite.  Every entry is one fixed-order expression.
//     graph_loop_candidates_kernel   one thread per frame i of the node table against ONE query q: dist = |t(T_i^-1 T_q)| and, unless the call
//                                    asks for distances only, sigma = sqrt(trace(Sigma_rel(i, q)[3:, 3:])) in the tangent at the stored relative
//                                    pose (rows 3 .. 5 of A and B alone), S_iq from the query's full column; the flag dist <= radius + k sigma
//     graph_loop_compact_kernel      ONE workgroup: the flagged frames in ascending order, by a prefix sum over 256 frames at a time; the first
//                                    `capacity` are written, the count is the total
struct GraphRel {
    const double* zenv;                          // as GraphCov
    double* work;                                // [n_cols][n_free][36]: the full columns
    const int* col_pos;                          // [n_cols]: the position whose block column a slot holds
    const int* pair;                             // [n_pairs][5]: frame a, frame b, free index of a, of b (-1: a constant), the slot of b's full column
                                                 // (-1: the cross block lies inside the envelope, or is zero)
    const double* z;                             // [n_pairs][6], or null: the stored relative pose
    const double* linfo;                         // [n_pairs][21], or null: the Cholesky factor of the pair's information, as GraphWeights::winfo
    double* out;                                 // [n_pairs][kGrRelOut]: rel (6), r (6), S (36), chi2
    int n_pairs;
};
constexpr int kGrRelOut = 49;

struct GraphCand {
    const double* zenv;
    const double* work;                          // [n_free][36]: the query's full column (not read for a constant query)
    const int* slot;                             // [n_frames]: -2 = no pose, -1 = a constant, otherwise the free index
    int* flag;                                   // [n_frames]
    double* rec;                                 // [n_frames][2]: dist, sigma
    double* out;                                 // the count, then per written candidate: frame, dist, sigma
    int n_frames, query, min_gap, capacity, with_sigma;
    double radius, k_sigma;
};

__global__ void __launch_bounds__(kGrEnvColumnThreads)
graph_env_column_full_kernel(GraphArgs G, GraphRel V)
#if VELO_DEF_GRAPH
{
    graph_env_column_body<true>(G, V.work, V.col_pos, 0);
}
#else
;
#endif

// entry (r, c) of Z_ab c_a c_b for the free indices ia, ib: off the skyline, or (col not null) off the full column of b's position
__device__ __forceinline__ double graph_rel_sigma(const GraphArgs& G, const double* zenv, const double* col, int ia, int ib, int r, int c) {
    const int pa = G.env_pos[ia], pb = G.env_pos[ib];
    double z;
    if (col) z = col[(size_t)pa * 36 + r * 6 + c];                    // row o of the column of q is Z(o, q)
    else {
        const int hi = pa > pb ? pa : pb, lo = pa > pb ? pb : pa;
        const double* B = zenv + ((size_t)G.env_rowptr[hi] + (size_t)(lo - G.env_first[hi])) * 36;
        z = pa >= pb ? B[r * 6 + c] : B[c * 6 + r];
    }
    return z * (G.scale[(size_t)ia * 6 + r] * G.scale[(size_t)ib * 6 + c]);
}

// rel = pose_vec(T_a^-1 T_b) from the 6 doubles of the two poses
__device__ __forceinline__ void graph_relative(const double* xa, const double* xb, double rel[6]) {
    const double wa[3] = {xa[0], xa[1], xa[2]}, wb[3] = {xb[0], xb[1], xb[2]};
    double Ra[9], Rb[9], Q[9];
    graph_rot_value(wa, Ra);
    graph_rot_value(wb, Rb);
    graph_mul3_tn(Ra, Rb, Q);
    graph_log(Q, rel);
    const double d[3] = {xb[3] - xa[3], xb[4] - xa[4], xb[5] - xa[5]};
#pragma unroll
    for (int i = 0; i < 3; i++) rel[3 + i] = Ra[i] * d[0] + Ra[3 + i] * d[1] + Ra[6 + i] * d[2];
}

__global__ void __launch_bounds__(64)
graph_relcov_kernel(GraphArgs G, GraphRel V)
#if VELO_DEF_GRAPH
{
    __shared__ double As[36], Bs[36], rs[6], Xs[36], Saa[36], Sab[36], Sbb[36], T1[36], T2[36], Ss[36];
    const int p = blockIdx.x, l = threadIdx.x;
    if (p >= V.n_pairs) return;
    const int* pr = V.pair + (size_t)p * 5;
    const int fa = pr[0], fb = pr[1], ia = pr[2], ib = pr[3], slot = pr[4];
    double* out = V.out + (size_t)p * kGrRelOut;
    if (l == 0) {                                                      // the stored state is buffer 0
        const double* xa = G.x + (size_t)fa * 6;
        const double* xb = G.x + (size_t)fb * 6;
        double rel[6], zz[6], r[6], A[36], B[36];
        graph_relative(xa, xb, rel);
#pragma unroll
        for (int k = 0; k < 6; k++) { zz[k] = V.z ? V.z[(size_t)p * 6 + k] : rel[k]; out[k] = rel[k]; }
        graph_edge_terms_at(xa, xb, zz, r, A, B);
#pragma unroll
        for (int k = 0; k < 36; k++) { As[k] = A[k]; Bs[k] = B[k]; }
#pragma unroll
        for (int k = 0; k < 6; k++) { rs[k] = r[k]; out[6 + k] = r[k]; }
    }
    if (l == 63) {                                                     // L^-1 of the pair's information; zero without one
        if (V.linfo) {
            double L[21];
#pragma unroll
            for (int k = 0; k < 21; k++) L[k] = V.linfo[(size_t)p * 21 + k];
            graph_env_inv6(L, Xs);
        } else {
#pragma unroll
            for (int k = 0; k < 36; k++) Xs[k] = 0.0;
        }
    }
    const int r = l / 6, c = l % 6;
    if (l < 36) {
        const bool ok = G.rec->bad == 0;
        Saa[l] = ia >= 0 && ok ? graph_rel_sigma(G, V.zenv, nullptr, ia, ia, r, c) : 0.0;
        Sbb[l] = ib >= 0 && ok ? graph_rel_sigma(G, V.zenv, nullptr, ib, ib, r, c) : 0.0;
        Sab[l] = ia >= 0 && ib >= 0 && ok ? graph_rel_sigma(G, V.zenv, slot >= 0 ? V.work + (size_t)slot * (size_t)G.n_free * 36 : nullptr, ia, ib, r, c) : 0.0;
    }
    __syncthreads();
    if (l < 36) {                                                      // T1 = S_aa A^T + S_ab B^T, T2 = S_ba A^T + S_bb B^T: entry (r, c)
        double t1 = 0.0, t2 = 0.0;
#pragma unroll
        for (int k = 0; k < 6; k++) t1 += Saa[r * 6 + k] * As[c * 6 + k];
#pragma unroll
        for (int k = 0; k < 6; k++) t1 += Sab[r * 6 + k] * Bs[c * 6 + k];
#pragma unroll
        for (int k = 0; k < 6; k++) t2 += Sab[k * 6 + r] * As[c * 6 + k];
#pragma unroll
        for (int k = 0; k < 6; k++) t2 += Sbb[r * 6 + k] * Bs[c * 6 + k];
        T1[l] = t1;
        T2[l] = t2;
    }
    __syncthreads();
    if (l < 36 && c <= r) {                                            // S = A T1 + B T2 + L^-T L^-1: the lower triangle, mirrored
        double s = 0.0, w = 0.0;
#pragma unroll
        for (int k = 0; k < 6; k++) s += As[r * 6 + k] * T1[k * 6 + c];
#pragma unroll
        for (int k = 0; k < 6; k++) s += Bs[r * 6 + k] * T2[k * 6 + c];
#pragma unroll
        for (int k = 0; k < 6; k++) w += Xs[k * 6 + r] * Xs[k * 6 + c];
        s += w;
        Ss[r * 6 + c] = s;
        Ss[c * 6 + r] = s;
        out[12 + r * 6 + c] = s;
        out[12 + c * 6 + r] = s;
    }
    __syncthreads();
    if (l == 0) {                                                      // chi2 = |L_S^-1 r|^2
        double M[36], y[6];
#pragma unroll
        for (int k = 0; k < 36; k++) M[k] = Ss[k];
        const bool ok = graph_chol6(M);
        double chi2 = 0.0;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            double s = rs[i];
#pragma unroll
            for (int k = 0; k < i; k++) s -= M[i * 6 + k] * y[k];
            y[i] = s / M[i * 6 + i];
            chi2 += y[i] * y[i];
        }
        out[48] = ok ? chi2 : -1.0;
    }
}
#else
;
#endif

__global__ void __launch_bounds__(kGrThreads)
graph_loop_candidates_kernel(GraphArgs G, GraphCand V)
#if VELO_DEF_GRAPH
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= V.n_frames) return;
    const int q = V.query, si = V.slot[i], sq = V.slot[q];
    const int gap = i > q ? i - q : q - i;
    double dist = 0.0, sigma = 0.0;
    int flag = 0;
    if (si != -2 && gap >= V.min_gap) {
        const double* xa = G.x + (size_t)i * 6;                        // the stored state is buffer 0
        const double* xb = G.x + (size_t)q * 6;
        double rel[6];
        graph_relative(xa, xb, rel);
        dist = sqrt(rel[3] * rel[3] + rel[4] * rel[4] + rel[5] * rel[5]);
        if (V.with_sigma) {
            double r[6], A[36], B[36];
            graph_edge_terms_at(xa, xb, rel, r, A, B);
            double tr = 0.0;
#pragma unroll
            for (int row = 3; row < 6; row++) {                        // a S_aa a^T + 2 a S_ab b^T + b S_bb b^T for the rows a, b of A, B
                double aa = 0.0, ab = 0.0, bb = 0.0;
#pragma unroll
                for (int k = 0; k < 6; k++) {
                    double s1 = 0.0, s2 = 0.0, s3 = 0.0;
#pragma unroll
                    for (int m = 0; m < 6; m++) {
                        if (si >= 0) s1 += graph_rel_sigma(G, V.zenv, nullptr, si, si, k, m) * A[row * 6 + m];
                        if (si >= 0 && sq >= 0) s2 += graph_rel_sigma(G, V.zenv, V.work, si, sq, k, m) * B[row * 6 + m];
                        if (sq >= 0) s3 += graph_rel_sigma(G, V.zenv, nullptr, sq, sq, k, m) * B[row * 6 + m];
                    }
                    aa += A[row * 6 + k] * s1;
                    ab += A[row * 6 + k] * s2;
                    bb += B[row * 6 + k] * s3;
                }
                tr += (aa + 2.0 * ab) + bb;
            }
            sigma = sqrt(fmax(tr, 0.0));
        }
        flag = dist <= V.radius + V.k_sigma * sigma ? 1 : 0;
    }
    V.flag[i] = flag;
    V.rec[(size_t)i * 2] = dist;
    V.rec[(size_t)i * 2 + 1] = sigma;
}
#else
;
#endif

constexpr int kGrCompactThreads = 256;
__global__ void __launch_bounds__(kGrCompactThreads)
graph_loop_compact_kernel(GraphCand V)
#if VELO_DEF_GRAPH
{
    __shared__ int cnt[kGrCompactThreads];
    const int t = threadIdx.x;
    int base = 0;
    for (int start = 0; start < V.n_frames; start += kGrCompactThreads) {
        const int i = start + t;
        const int f = i < V.n_frames ? V.flag[i] : 0;
        cnt[t] = f;
        __syncthreads();
        for (int off = 1; off < kGrCompactThreads; off <<= 1) {        // an inclusive prefix sum of the flags
            const int v = t >= off ? cnt[t - off] : 0;
            __syncthreads();
            cnt[t] += v;
            __syncthreads();
        }
        const int at = base + cnt[t] - f;
        if (f && at < V.capacity) {
            V.out[1 + (size_t)at * 3] = (double)i;
            V.out[2 + (size_t)at * 3] = V.rec[(size_t)i * 2];
            V.out[3 + (size_t)at * 3] = V.rec[(size_t)i * 2 + 1];
        }
        base += cnt[kGrCompactThreads - 1];
        __syncthreads();
    }
    if (t == 0) V.out[0] = (double)base;
}
#else
;
#endif

}  // namespace velo
