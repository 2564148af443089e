// velo_ba_kernels.h -- bundle adjustment of a window of frames over the resident landmark store (reference main.cpp:673-725, the functors
// bundle2D / bundle3D of costfunctions.h:222-286).  Included by velo_hip.hip (declarations) and by velo_unit_ba.hip (VELO_DEF_BA: the
// definitions); gfx950 only.
//
// Unknowns: the 6 doubles of every FREE frame of the window and the 3 doubles of every participating landmark.  The solver is the
// trust-region Levenberg-Marquardt of SURVEY.md B1 (the controller of velo_trust_region.h) over all of them; its linear step is the
// Schur complement on the landmark blocks.  With H = [U W; W^T V] the Jacobi-scaled J^T J, D the clipped diagonal and mu the radius:
//     A_l = V_l + D_l / mu                                   3 x 3 per landmark, solved with tri_chol3
//     S   = U + D_c / mu - sum_l W_l A_l^-1 W_l^T            6 n_free square, factored by ONE workgroup in LDS
//     S y_c = g_c - sum_l W_l A_l^-1 g_l,  s_c = -y_c,  s_l = A_l^-1 (-g_l - W_l^T s_c)
// One LM iteration is five launches (the host reads one 64-byte record after them):
//     ba_schur_kernel      one workgroup per upper block (k, m) of sum W A^-1 W^T and per block of sum W A^-1 g: a fixed tree over landmarks
//     ba_solve_kernel      one workgroup: assembles and factors S, the pose step, the candidate poses, the poses' share of the model change
//     ba_linearize_kernel  one wave per landmark: back-substitution -> candidate point, then the linearisation AT the candidate
//                          (one lane per observation, robustified rows to LDS, every accumulator summed in block order by one lane)
//     ba_reduce_kernel     one workgroup per scalar: U and g_c of every free frame, cost, model change, norms, gradient maximum
//     ba_decide_kernel     the B1 transition: accept (the candidate buffers become the current ones) / reject, radius, termination
// Every sum has a fixed order and nothing is accumulated with atomics, so two identical calls give identical bytes.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/velo_hip.h"
#include "velo_scan_types.h"
#include "velo_tri_kernels.h"
#include "velo_landmark_kernels.h"

#ifndef VELO_DEF_BA
#define VELO_DEF_BA 0
#endif

namespace velo {

constexpr int kBaMaxFree = 10;
constexpr int kBaMaxObs = 64;                    // n_frames x n_cams <= 64: a landmark's window observations fit one wave
constexpr int kBaBlk = 45;                       // per (landmark, free frame): W 6x3 (18), upper U 6x6 (21), g_c (6)
constexpr int kBaLin = 10;                       // per landmark: upper V (6), g_p (3), cost
constexpr int kBaRed = 27;                       // per free frame, reduced over landmarks: upper U (21), g_c (6)
constexpr int kBaScalars = 5;                    // cost, model change, |step|^2, |x|^2, gradient maximum (points' share)

struct BaWindow { int frames[kBaMaxObs]; int n_frames, n_fixed, n_free, n_cams; };

struct BaRecord {                                // what the host reads after every iteration: 64 bytes
    int status, iteration, done, termination;
    double cost, candidate_cost, radius, model_change, step_norm;
    int evaluations, pad;
};

struct BaState {
    BaRecord rec;
    TrustRegion tr;
    double pose_model, pose_dn2, pose_xn2[2];
    int cur, step_ok, bad, pad;
    double scale_c[6 * kBaMaxFree], diag_c[6 * kBaMaxFree], step_c[6 * kBaMaxFree], delta_c[6 * kBaMaxFree];
};

struct BaArgs {
    // the store
    const TriFrame* frames; const double* cam_t; const velo_tri_obs* log; const int* prev; const int* head; float* pts; const unsigned char* added;
    // the call
    const int* cand_ids; int n_cand;
    velo_tri_obs* obs;          // [n_cand][64]: a candidate's window observations in block order, .frame = index into the window
    int* n_obs;                 // [n_cand]: how many, 0 for a landmark that does not take part
    int* n_3d;                  // [n_cand]
    int* sel;                   // [L] -> candidate
    int* hdr;                   // L, blocks, residuals
    BaState* st;
    double* xc;                 // [2][n_frames][6] poses, current / candidate
    double* pt;                 // [2][L][3]
    double* lin;                // [2][L][10]
    double* blk;                // [2][L][n_free][45]
    double* scale_p; double* diag_p;    // [L][3]
    double* lterm;              // [L][4]: model change, |step|^2, |x|^2
    unsigned* fmask;            // [L]: the free frames that observe the landmark
    double* red;                // [2][n_free * 27 + 5]
    double* sch;                // [pairs][36] then [n_free][6]
    int L;
    BaWindow W;
    TriParams P;
    double weight_3d;
};

__device__ __forceinline__ int ba_pair(int k, int m, int n) { return k * n - (k * (k - 1)) / 2 + (m - k); }   // k <= m < n

// ---- selection -------------------------------------------------------------------------------------------------------------
// One wave per candidate id (the ascending union of what the window's frames observed): walks the landmark's chain like
// lm_gather_kernel, keeps the entries whose frame is in the window and writes them in block order (lm_order_key).
__device__ __forceinline__ int ba_window_index(const BaWindow& W, int frame) {
    int lo = 0, hi = W.n_frames - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1, f = W.frames[mid];
        if (f == frame) return mid;
        if (f < frame) lo = mid + 1; else hi = mid - 1;
    }
    return -1;
}

__global__ void __launch_bounds__(64)
ba_gather_kernel(BaArgs A)
#if VELO_DEF_BA
{
    const int c = blockIdx.x;
    if (c >= A.n_cand) return;
    const int lane = threadIdx.x;
    const int id = A.cand_ids[c];
    const int first = A.head[id];
    int cur = first, n_win = 0, n_free = 0, n_3d = 0;
    while (cur >= 0) {
        int mine = -1, p = cur;
        for (int k = 0; k < 64 && p >= 0; k++) {
            if (k == lane) mine = p;
            p = A.prev[p];
        }
        cur = p;
        bool in_w = false;
        int wi = -1;
        velo_tri_obs o;
        o.kind = 0;
        if (mine >= 0) {
            o = A.log[mine];
            wi = ba_window_index(A.W, o.frame);
            in_w = wi >= 0;
        }
        if (in_w) {
            const unsigned long long key = lm_order_key(o);
            int rank = 0;
            for (int q = first; q >= 0; q = A.prev[q]) {
                const velo_tri_obs oq = A.log[q];
                rank += (ba_window_index(A.W, oq.frame) >= 0 && lm_order_key(oq) < key) ? 1 : 0;
            }
            o.frame = wi;
            if (rank < kBaMaxObs) A.obs[(size_t)c * kBaMaxObs + rank] = o;
        }
        n_win += (int)__popcll(__ballot(in_w));
        n_free += (int)__popcll(__ballot(in_w && wi >= A.W.n_fixed));
        n_3d += (int)__popcll(__ballot(in_w && o.kind == VELO_TRI_OBS_3D));
    }
    if (lane == 0) {
        const bool takes_part = A.added[id] != 0 && n_win >= 2 && n_free >= 1 && n_win <= kBaMaxObs;
        A.n_obs[c] = takes_part ? n_win : 0;
        A.n_3d[c] = takes_part ? n_3d : 0;
    }
}
#else
;
#endif

// One workgroup: the participating candidates in ascending order, the counts the host reads, the poses of the window, the points
// widened from the stored float, the start of the LM state.
__global__ void __launch_bounds__(256)
ba_compact_kernel(BaArgs A, int L_cap)
#if VELO_DEF_BA
{
    __shared__ int cnt[256], blocks[256], res[256], base[256];
    const int t = threadIdx.x;
    const int per = (A.n_cand + 255) / 256;
    const int lo = min(t * per, A.n_cand), hi = min(lo + per, A.n_cand);
    int n = 0, nb = 0, nr = 0;
    for (int c = lo; c < hi; c++) {
        const int m = A.n_obs[c];
        if (m > 0) { n++; nb += m; nr += 3 * A.n_3d[c] + 2 * (m - A.n_3d[c]); }
    }
    cnt[t] = n; blocks[t] = nb; res[t] = nr;
    __syncthreads();
    if (t == 0) {
        int s = 0, sb = 0, sr = 0;
        for (int k = 0; k < 256; k++) { base[k] = s; s += cnt[k]; sb += blocks[k]; sr += res[k]; }
        A.hdr[0] = s; A.hdr[1] = sb; A.hdr[2] = sr;
        BaState* st = A.st;
        st->cur = 0; st->step_ok = 0; st->bad = 0;                    // (ba_decide_kernel starts st->tr)
        st->rec.status = 0; st->rec.iteration = 0; st->rec.done = 0; st->rec.termination = VELO_NO_CONVERGENCE; st->rec.evaluations = 0;
    }
    __syncthreads();
    int w = base[t];
    for (int c = lo; c < hi; c++)
        if (A.n_obs[c] > 0) { if (w < L_cap) A.sel[w] = c; w++; }
    for (int i = t; i < A.W.n_frames * 6; i += 256) {
        const TriFrame& F = A.frames[A.W.frames[i / 6]];
        const int j = i % 6;
        const double v = j < 3 ? -F.w[j] : F.center[j - 3];           // TriFrame keeps -omega and the centre: the pose, exactly
        A.xc[i] = v;
        A.xc[A.W.n_frames * 6 + i] = v;
    }
}
#else
;
#endif

__global__ void __launch_bounds__(256)
ba_points_in_kernel(BaArgs A)
#if VELO_DEF_BA
{
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= A.L) return;
    const int id = A.cand_ids[A.sel[l]];
#pragma unroll
    for (int j = 0; j < 3; j++) A.pt[3 * (size_t)l + j] = (double)A.pts[3 * (size_t)id + j];
}
#else
;
#endif

__global__ void __launch_bounds__(256)
ba_points_out_kernel(BaArgs A)
#if VELO_DEF_BA
{
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= A.L) return;
    const int id = A.cand_ids[A.sel[l]];
    const double* p = A.pt + ((size_t)A.st->cur * A.L + l) * 3;
#pragma unroll
    for (int j = 0; j < 3; j++) A.pts[3 * (size_t)id + j] = (float)p[j];
}
#else
;
#endif

// ---- linearisation ---------------------------------------------------------------------------------------------------------
// The robustified rows of one observation at (camera, point): row q = {d r_q / d point (3), d r_q / d camera (6), r_q} * sqrt(rho').
// bundle3D / bundle2D with rot = -camera[0..2] through pose_rot_init / rotate_point (velo_device_math.h): the value is the Rodrigues
// form tri_rotate follows, sin and cos come from velo_sincos, the partials are those of the dual-number evaluation.
__device__ __forceinline__ int ba_obs_rows(const double* cam, const velo_tri_obs& o, const double* cam_t, double weight_3d, const TriParams& P,
                                           const double x[3], double rows[3][10], double* half_rho) {
    const double w[3] = {-cam[0], -cam[1], -cam[2]};
    PoseRot R;
    pose_rot_init(w, &R);
    const double m0[3] = {x[0] - cam[3], x[1] - cam[4], x[2] - cam[5]};
    D3 m[3];
    rotate_point(R, m0, m);
    double Rm[3][3];                                                  // column j = rotation of e_j = d M / d point_j
#pragma unroll
    for (int j = 0; j < 3; j++) {
        const double e[3] = {j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0};
        double col[3];
        rotate_point_value(R, e, col);
        Rm[0][j] = col[0]; Rm[1][j] = col[1]; Rm[2][j] = col[2];
    }
    double r[3], J[3][9], rho0, rho1;
    int d;
    if (o.kind == VELO_TRI_OBS_3D) {
        d = 3;
#pragma unroll
        for (int q = 0; q < 3; q++) {
            r[q] = weight_3d * (m[q].a - (double)o.s[q]);
#pragma unroll
            for (int j = 0; j < 3; j++) { J[q][j] = weight_3d * Rm[q][j]; J[q][3 + j] = weight_3d * (-m[q].v[j]); J[q][6 + j] = weight_3d * (-Rm[q][j]); }
        }
        rho0 = r[0] * r[0] + r[1] * r[1] + r[2] * r[2]; rho1 = 1.0;     // TrivialLoss
    } else {
        d = 2;
        const double sx = (double)o.s[0], sy = (double)o.s[1];
        const double M0 = m[0].a + cam_t[3 * o.cam], M1 = m[1].a + cam_t[3 * o.cam + 1], M2 = m[2].a + cam_t[3 * o.cam + 2];
        r[0] = M0 - sx * M2;
        r[1] = M1 - sy * M2;
        r[2] = 0.0;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double d0 = -m[0].v[j], d1 = -m[1].v[j], d2 = -m[2].v[j];
            J[0][j] = Rm[0][j] - sx * Rm[2][j];     J[1][j] = Rm[1][j] - sy * Rm[2][j];     J[2][j] = 0.0;
            J[0][3 + j] = d0 - sx * d2;             J[1][3 + j] = d1 - sy * d2;             J[2][3 + j] = 0.0;
            J[0][6 + j] = -Rm[0][j] - sx * (-Rm[2][j]); J[1][6 + j] = -Rm[1][j] - sy * (-Rm[2][j]); J[2][6 + j] = 0.0;
        }
        loss_cauchy(P.loss_a, P.loss_w, r[0] * r[0] + r[1] * r[1], &rho0, &rho1);
    }
    *half_rho = 0.5 * rho0;
    const double sr = sqrt(rho1);
#pragma unroll
    for (int q = 0; q < 3; q++) {
#pragma unroll
        for (int j = 0; j < 9; j++) rows[q][j] = J[q][j] * sr;
        rows[q][9] = r[q] * sr;
    }
    return d;
}

// the two columns of a row whose products accumulator e of a (landmark, free frame) record sums: W, upper U, g_c
__device__ __forceinline__ void ba_blk_columns(int e, int* ca, int* cb) {
    if (e < 18) { *ca = 3 + e / 3; *cb = e % 3; }
    else if (e < 39) {
        int t = e - 18, i = 0;
        while (t >= 6 - i) { t -= 6 - i; i++; }
        *ca = 3 + i; *cb = 3 + i + t;
    } else { *ca = 3 + (e - 39); *cb = 9; }
}

// the landmark's own accumulators: upper V, g_p
__device__ __forceinline__ void ba_lin_columns(int a, int* ca, int* cb) {
    if (a < 3) { *ca = 0; *cb = a; }
    else if (a < 5) { *ca = 1; *cb = a - 2; }
    else if (a == 5) { *ca = 2; *cb = 2; }
    else { *ca = a - 6; *cb = 9; }
}

struct BaShared {
    double rows[kBaMaxObs * 3][10];
    double half_rho[kBaMaxObs];
    int widx[kBaMaxObs], dim[kBaMaxObs];
};

// A_l = c V c + D / mu of one landmark (upper V in v[0..5]); refresh: D = clip(diag(c V c)) as B1 does after an accepted step
__device__ __forceinline__ void ba_point_block(const double* v, const double* cp, double* dp, bool refresh, double mu, const LMParams& Q,
                                               double Vs[9], double A3[9]) {
    const double V[9] = {v[0], v[1], v[2], v[1], v[3], v[4], v[2], v[4], v[5]};
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
        for (int j = 0; j < 3; j++) Vs[i * 3 + j] = V[i * 3 + j] * cp[i] * cp[j];
    }
    if (refresh) {
#pragma unroll
        for (int j = 0; j < 3; j++) dp[j] = fmin(fmax(Vs[j * 3 + j], Q.min_diag), Q.max_diag);
    }
#pragma unroll
    for (int i = 0; i < 9; i++) A3[i] = Vs[i];
#pragma unroll
    for (int j = 0; j < 3; j++) { const double l = sqrt(dp[j] / mu); A3[j * 3 + j] += l * l; }
}

// mode 0: linearise at the current state into the current buffers (the start of a call).  mode 1: back-substitute the pose step into
// the landmark's step, form the candidate point and linearise at the candidate into the other buffers.
__global__ void __launch_bounds__(64)
ba_linearize_kernel(BaArgs A, int mode)
#if VELO_DEF_BA
{
    __shared__ BaShared sh;
    const int l = blockIdx.x;
    if (l >= A.L) return;
    const int lane = threadIdx.x;
    const BaState* st = A.st;
    const int src = st->cur, dst = mode == 0 ? src : src ^ 1;
    const int c = A.sel[l], n_obs = A.n_obs[c], n3d = A.n_3d[c], nf = A.W.n_free;
    const size_t L = (size_t)A.L;
    double x[3];
#pragma unroll
    for (int j = 0; j < 3; j++) x[j] = A.pt[(src * L + l) * 3 + j];
    double term[3] = {0.0, 0.0, 0.0};
    if (mode == 1) {                                                  // wave-uniform: every lane does the same arithmetic
        const double* v = A.lin + (src * L + l) * kBaLin;
        const double cp[3] = {A.scale_p[3 * l], A.scale_p[3 * l + 1], A.scale_p[3 * l + 2]};
        double dp[3] = {A.diag_p[3 * l], A.diag_p[3 * l + 1], A.diag_p[3 * l + 2]};
        double Vs[9], A3[9];
        ba_point_block(v, cp, dp, st->tr.refresh != 0, st->tr.radius, A.P.lm, Vs, A3);
        if (st->tr.refresh != 0 && lane == 0) { A.diag_p[3 * l] = dp[0]; A.diag_p[3 * l + 1] = dp[1]; A.diag_p[3 * l + 2] = dp[2]; }
        double ws[3] = {0.0, 0.0, 0.0};                               // W^T (pose step), unscaled
        const unsigned mask = A.fmask[l];
        for (int k = 0; k < nf; k++) {
            if (!((mask >> k) & 1u)) continue;
            const double* Wk = A.blk + ((src * L + l) * nf + k) * kBaBlk;
            for (int i = 0; i < 6; i++) {
                const double dc = st->delta_c[6 * k + i];
#pragma unroll
                for (int j = 0; j < 3; j++) ws[j] += Wk[3 * i + j] * dc;
            }
        }
        double gs[3], b[3], sp[3];
#pragma unroll
        for (int j = 0; j < 3; j++) { gs[j] = v[6 + j] * cp[j]; ws[j] *= cp[j]; b[j] = -gs[j] - ws[j]; }
        if (!tri_chol3(A3, b, sp)) {
            sp[0] = 0.0; sp[1] = 0.0; sp[2] = 0.0;
            if (lane == 0) atomicOr(&A.st->bad, 1);
        }
        double gd = 0.0, cross = 0.0, quad = 0.0, dn2 = 0.0;
#pragma unroll
        for (int i = 0; i < 3; i++) {
            gd += gs[i] * sp[i];
            cross += ws[i] * sp[i];
#pragma unroll
            for (int j = 0; j < 3; j++) quad += sp[i] * Vs[i * 3 + j] * sp[j];
            const double d = sp[i] * cp[i];
            x[i] += d;
            dn2 += d * d;
        }
        term[0] = gd + 0.5 * (2.0 * cross + quad);
        term[1] = dn2;
    }
    term[2] = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
    if (lane == 0) {
        if (mode == 1) { A.pt[(dst * L + l) * 3] = x[0]; A.pt[(dst * L + l) * 3 + 1] = x[1]; A.pt[(dst * L + l) * 3 + 2] = x[2]; }
        A.lterm[4 * l] = term[0]; A.lterm[4 * l + 1] = term[1]; A.lterm[4 * l + 2] = term[2];
    }
    if (lane < n_obs) {
        const velo_tri_obs o = A.obs[(size_t)c * kBaMaxObs + lane];
        const double* cam = A.xc + ((size_t)dst * A.W.n_frames + o.frame) * 6;
        double rows[3][10], hr;
        const int d = ba_obs_rows(cam, o, A.cam_t, A.weight_3d, A.P, x, rows, &hr);
        const int r0 = tri_row_of(lane, n3d);
#pragma unroll
        for (int q = 0; q < 3; q++) {
            if (q < d) {
#pragma unroll
                for (int j = 0; j < 10; j++) sh.rows[r0 + q][j] = rows[q][j];
            }
        }
        sh.half_rho[lane] = hr; sh.widx[lane] = o.frame; sh.dim[lane] = d;
    }
    __syncthreads();
    if (mode == 0) {
        if (lane == 0) {
            unsigned m = 0;
            for (int p = 0; p < n_obs; p++) if (sh.widx[p] >= A.W.n_fixed) m |= 1u << (sh.widx[p] - A.W.n_fixed);
            A.fmask[l] = m;
        }
    }
    const int n_rows = tri_row_of(n_obs, n3d);
    double* lin = A.lin + (dst * L + l) * kBaLin;
    double* blk = A.blk + (dst * L + l) * nf * kBaBlk;
    for (int a = lane; a < kBaLin + nf * kBaBlk; a += 64) {
        double acc = 0.0;
        if (a < 9) {
            int ca, cb;
            ba_lin_columns(a, &ca, &cb);
            for (int r = 0; r < n_rows; r++) acc += sh.rows[r][ca] * sh.rows[r][cb];
            lin[a] = acc;
        } else if (a == 9) {
            for (int p = 0; p < n_obs; p++) acc += sh.half_rho[p];
            lin[a] = acc;
        } else {
            const int k = (a - kBaLin) / kBaBlk, e = (a - kBaLin) % kBaBlk;
            int ca, cb;
            ba_blk_columns(e, &ca, &cb);
            for (int p = 0; p < n_obs; p++) {
                if (sh.widx[p] != A.W.n_fixed + k) continue;
                const int r0 = tri_row_of(p, n3d);
                for (int q = 0; q < sh.dim[p]; q++) acc += sh.rows[r0 + q][ca] * sh.rows[r0 + q][cb];
            }
            blk[k * kBaBlk + e] = acc;
        }
    }
    if (mode == 0 && lane < 3) {                                      // Jacobi scaling, once (B1)
        double acc = 0.0;                                             // V_jj, summed as its accumulator above sums it
        for (int r = 0; r < n_rows; r++) acc += sh.rows[r][lane] * sh.rows[r][lane];
        A.scale_p[3 * l + lane] = 1.0 / (1.0 + sqrt(acc));
    }
}
#else
;
#endif

// ---- reductions over landmarks: thread t sums the landmarks t, t + 256, ... in order, then a fixed tree over the 256 partial sums -----
__device__ __forceinline__ double ba_tree_sum(double* buf, double v) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) buf[t] += buf[t + s];
        __syncthreads();
    }
    const double out = buf[0];
    __syncthreads();
    return out;
}

__device__ __forceinline__ double ba_tree_max(double* buf, double v) {
    const int t = threadIdx.x;
    buf[t] = v;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) buf[t] = fmax(buf[t], buf[t + s]);
        __syncthreads();
    }
    const double out = buf[0];
    __syncthreads();
    return out;
}

// which = 0: the current buffers, 1: the candidate's
__global__ void __launch_bounds__(256)
ba_reduce_kernel(BaArgs A, int which)
#if VELO_DEF_BA
{
    __shared__ double buf[256];
    const int t = threadIdx.x, idx = blockIdx.x, nf = A.W.n_free;
    const int b = which == 0 ? A.st->cur : A.st->cur ^ 1;
    const size_t L = (size_t)A.L;
    double* out = A.red + (size_t)b * (nf * kBaRed + kBaScalars);
    double acc = 0.0;
    if (idx < nf * kBaRed) {
        const int k = idx / kBaRed, e = 18 + idx % kBaRed;
        for (size_t l = t; l < L; l += 256) acc += A.blk[((b * L + l) * nf + k) * kBaBlk + e];
    } else {
        const int s = idx - nf * kBaRed;
        if (s == 0) { for (size_t l = t; l < L; l += 256) acc += A.lin[(b * L + l) * kBaLin + 9]; }
        else if (s < 4) { for (size_t l = t; l < L; l += 256) acc += A.lterm[4 * l + (s - 1)]; }
        else {
            for (size_t l = t; l < L; l += 256) {
                const double* g = A.lin + (b * L + l) * kBaLin + 6;
                acc = fmax(acc, fmax(fmax(fabs(g[0]), fabs(g[1])), fabs(g[2])));
            }
            const double m = ba_tree_max(buf, acc);
            if (t == 0) out[idx] = m;
            return;
        }
    }
    const double s = ba_tree_sum(buf, acc);
    if (t == 0) out[idx] = s;
}
#else
;
#endif

// sum_l W_k B_l W_m^T for one upper pair (k, m) of free frames, B_l = c (c V c + D / mu)^-1 c; after the pairs, sum_l W_k B_l g_l per frame.
// The poses' own scaling factors out of the sums and is applied by ba_solve_kernel.
__global__ void __launch_bounds__(256)
ba_schur_kernel(BaArgs A)
#if VELO_DEF_BA
{
    __shared__ double buf[256];
    const int t = threadIdx.x, nf = A.W.n_free;
    const int n_pairs = nf * (nf + 1) / 2;
    const BaState* st = A.st;
    const int cur = st->cur;
    const bool refresh = st->tr.refresh != 0;
    const double mu = st->tr.radius;
    const size_t L = (size_t)A.L;
    int k = 0, m = 0;
    const bool rhs = (int)blockIdx.x >= n_pairs;
    if (rhs) { k = blockIdx.x - n_pairs; m = k; }
    else {
        int p = blockIdx.x;
        while (p >= nf - k) { p -= nf - k; k++; }
        m = k + p;
    }
    double acc[36];
#pragma unroll
    for (int i = 0; i < 36; i++) acc[i] = 0.0;
    for (size_t l = t; l < L; l += 256) {
        const unsigned mask = A.fmask[l];
        if (!((mask >> k) & 1u) || !((mask >> m) & 1u)) continue;
        const double* v = A.lin + (cur * L + l) * kBaLin;
        const double cp[3] = {A.scale_p[3 * l], A.scale_p[3 * l + 1], A.scale_p[3 * l + 2]};
        double dp[3] = {A.diag_p[3 * l], A.diag_p[3 * l + 1], A.diag_p[3 * l + 2]};
        double Vs[9], A3[9], B[9];
        ba_point_block(v, cp, dp, refresh, mu, A.P.lm, Vs, A3);
        bool ok = true;
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double e[3] = {j == 0 ? 1.0 : 0.0, j == 1 ? 1.0 : 0.0, j == 2 ? 1.0 : 0.0};
            double col[3];
            ok = tri_chol3(A3, e, col) && ok;
            B[0 * 3 + j] = col[0] * cp[0] * cp[j]; B[1 * 3 + j] = col[1] * cp[1] * cp[j]; B[2 * 3 + j] = col[2] * cp[2] * cp[j];
        }
        if (!ok) continue;                                            // ba_linearize_kernel flags the step invalid
        const double* Wk = A.blk + ((cur * L + l) * nf + k) * kBaBlk;
        if (rhs) {
            double z[3];
#pragma unroll
            for (int i = 0; i < 3; i++) z[i] = B[i * 3] * v[6] + B[i * 3 + 1] * v[7] + B[i * 3 + 2] * v[8];
#pragma unroll
            for (int i = 0; i < 6; i++) acc[i] += Wk[3 * i] * z[0] + Wk[3 * i + 1] * z[1] + Wk[3 * i + 2] * z[2];
        } else {
            const double* Wm = A.blk + ((cur * L + l) * nf + m) * kBaBlk;
#pragma unroll
            for (int i = 0; i < 6; i++) {
                double T[3];
#pragma unroll
                for (int q = 0; q < 3; q++) T[q] = Wk[3 * i] * B[q] + Wk[3 * i + 1] * B[3 + q] + Wk[3 * i + 2] * B[6 + q];
#pragma unroll
                for (int j = 0; j < 6; j++) acc[i * 6 + j] += T[0] * Wm[3 * j] + T[1] * Wm[3 * j + 1] + T[2] * Wm[3 * j + 2];
            }
        }
    }
    if (rhs) {
        double* out = A.sch + (size_t)n_pairs * 36 + 6 * k;
#pragma unroll
        for (int i = 0; i < 6; i++) { const double s = ba_tree_sum(buf, acc[i]); if (t == 0) out[i] = s; }
    } else {
        double* out = A.sch + (size_t)blockIdx.x * 36;
#pragma unroll
        for (int i = 0; i < 36; i++) { const double s = ba_tree_sum(buf, acc[i]); if (t == 0) out[i] = s; }
    }
}
#else
;
#endif

// ---- the reduced system: one workgroup, everything in LDS ----------------------------------------------------------------------
__global__ void __launch_bounds__(64)
ba_solve_kernel(BaArgs A)
#if VELO_DEF_BA
{
    constexpr int N = 6 * kBaMaxFree;
    __shared__ double S[N][N + 1], rhs[N], y[N], gs[N], us[N], sc[N], dlt[N], xn[N];
    __shared__ int ok_s;
    const int i = threadIdx.x, nf = A.W.n_free, n = 6 * nf;
    BaState* st = A.st;
    const int cur = st->cur;
    const int n_pairs = nf * (nf + 1) / 2;
    const double* red = A.red + (size_t)cur * (nf * kBaRed + kBaScalars);
    const double mu = st->tr.radius;
    if (i == 0) { ok_s = 1; st->bad = 0; }
    if (i < n) sc[i] = st->scale_c[i];
    __syncthreads();
    if (i < n) {
        const int k = i / 6, a = i % 6;
        const double* U = red + k * kBaRed;
        const double ci = sc[i];
        double di = st->diag_c[i];
        if (st->tr.refresh) { di = fmin(fmax(U[upper6(a, a)] * ci * ci, A.P.lm.min_diag), A.P.lm.max_diag); st->diag_c[i] = di; }
        for (int j = 0; j < n; j++) {
            const int m = j / 6, b = j % 6;
            double val = k == m ? U[upper6(min(a, b), max(a, b))] : 0.0;
            const double e = k <= m ? A.sch[(size_t)ba_pair(k, m, nf) * 36 + a * 6 + b] : A.sch[(size_t)ba_pair(m, k, nf) * 36 + b * 6 + a];
            val -= e;
            S[i][j] = val * ci * sc[j];
        }
        const double lam = sqrt(di / mu);
        S[i][i] += lam * lam;
        gs[i] = U[21 + a] * ci;
        rhs[i] = (U[21 + a] - A.sch[(size_t)n_pairs * 36 + i]) * ci;
    }
    __syncthreads();
    // the off-diagonal blocks of S come from a sum whose (k, m) and (m, k) entries are the same number; the diagonal blocks are symmetrised
    // by reading the upper triangle
    if (i < n) for (int j = 0; j < i; j++) S[i][j] = S[j][i];
    __syncthreads();
    // Cholesky, right-looking: thread i owns row i.  Column j is scaled, then every row subtracts its share from the trailing
    // columns -- independent updates, so the LDS latency overlaps; every entry still sees its subtractions in ascending column order,
    // the order of the textbook left-looking loop.  L overwrites the lower triangle.
    for (int j = 0; j < n; j++) {
        double djj = S[j][j];
        if (!(djj > 0.0) || !isfinite(djj)) { if (i == 0) ok_s = 0; djj = 1.0; }
        const double ljj = sqrt(djj);
        const bool below = i > j && i < n;
        const double lij = below ? S[i][j] / ljj : 0.0;
        __syncthreads();
        if (i == j) S[j][j] = ljj;
        if (below) S[i][j] = lij;
        __syncthreads();
        if (below) for (int k = j + 1; k <= i; k++) S[i][k] -= lij * S[k][j];
        __syncthreads();
    }
    // L z = rhs, column by column; then L^T y = z from the last row up
    double acc = i < n ? rhs[i] : 0.0;
    for (int q = 0; q < n; q++) {
        if (i == q) y[q] = acc / S[q][q];
        __syncthreads();
        if (i > q && i < n) acc -= S[i][q] * y[q];
    }
    __syncthreads();
    acc = i < n ? y[i] : 0.0;
    for (int q = n - 1; q >= 0; q--) {
        if (i == q) y[q] = acc / S[q][q];
        __syncthreads();
        if (i < q) acc -= S[q][i] * y[q];
    }
    __syncthreads();
    if (i < n && !isfinite(y[i])) ok_s = 0;
    __syncthreads();
    const bool ok = ok_s != 0;
    const int nfr = A.W.n_frames, nfx = A.W.n_fixed;
    if (i < n) {                                                      // the step, the candidate pose
        const double s = ok ? -y[i] : 0.0, d = s * sc[i];
        y[i] = s;
        st->step_c[i] = s;
        st->delta_c[i] = d;
        dlt[i] = d;
        const double v = A.xc[((size_t)cur * nfr + nfx) * 6 + i] + d;
        xn[i] = v;
        A.xc[((size_t)(cur ^ 1) * nfr + nfx) * 6 + i] = v;
    }
    for (int r = i; r < 6 * nfx; r += 64) A.xc[(size_t)(cur ^ 1) * nfr * 6 + r] = A.xc[(size_t)cur * nfr * 6 + r];
    __syncthreads();
    if (i < n) {                                                      // row i of (c U c) s: the poses' share of s^T H s
        const int k = i / 6, a = i % 6;
        const double* U = red + k * kBaRed;
        double s = 0.0;
        for (int b = 0; b < 6; b++) s += U[upper6(min(a, b), max(a, b))] * sc[i] * sc[6 * k + b] * y[6 * k + b];
        us[i] = s;
    }
    __syncthreads();
    if (i == 0) {
        double gd = 0.0, quad = 0.0, dn2 = 0.0, xn2 = 0.0;
        for (int r = 0; r < n; r++) {
            gd += gs[r] * y[r];
            quad += y[r] * us[r];
            dn2 += dlt[r] * dlt[r];
            xn2 += xn[r] * xn[r];
        }
        st->pose_model = gd + 0.5 * quad;
        st->pose_dn2 = dn2;
        st->pose_xn2[cur ^ 1] = xn2;
        st->step_ok = ok ? 1 : 0;
    }
}
#else
;
#endif

// ---- the B1 transition: velo_trust_region.h on the reduced numbers -------------------------------------------------------------
// mode 0: after the first linearisation.  mode 1: after a candidate has been linearised and reduced.
__global__ void __launch_bounds__(64)
ba_decide_kernel(BaArgs A, int mode)
#if VELO_DEF_BA
{
    if (threadIdx.x != 0) return;
    BaState* st = A.st;
    const LMParams& Q = A.P.lm;
    const int nf = A.W.n_free, n = 6 * nf, stride = nf * kBaRed + kBaScalars;
    BaRecord& R = st->rec;
    TrustRegion T = st->tr;
    auto gradient_max = [&](const double* red) {
        double g = red[nf * kBaRed + 4];
        for (int k = 0; k < nf; k++) for (int a = 0; a < 6; a++) g = fmax(g, fabs(red[k * kBaRed + 21 + a]));
        return g;
    };
    R.candidate_cost = 0.0; R.model_change = 0.0; R.step_norm = 0.0;
    if (mode == 0) {
        const double* red = A.red + (size_t)st->cur * stride;
        double xn2 = 0.0;
        for (int r = 0; r < n; r++) { const double v = A.xc[((size_t)st->cur * A.W.n_frames + A.W.n_fixed) * 6 + r]; xn2 += v * v; }
        st->pose_xn2[st->cur] = xn2;
        for (int k = 0; k < nf; k++) for (int a = 0; a < 6; a++) st->scale_c[6 * k + a] = 1.0 / (1.0 + sqrt(red[k * kBaRed + upper6(a, a)]));
        tr_start(Q, &T, red[nf * kBaRed], sqrt(xn2 + red[nf * kBaRed + 3]), gradient_max(red));
        R.iteration = 0; R.status = 0; R.cost = T.cost; R.radius = T.radius;
    } else {
        const int cand = st->cur ^ 1;
        const double* red = A.red + (size_t)cand * stride;
        R.iteration = T.iteration; R.cost = T.cost; R.radius = T.radius;
        const double model_change = -(st->pose_model + red[nf * kBaRed + 1]);
        const bool ok = st->step_ok != 0 && st->bad == 0 && model_change > 0.0 && isfinite(model_change);
        if (!ok) R.status = tr_invalid(Q, &T);
        else {
            const double dn = sqrt(st->pose_dn2 + red[nf * kBaRed + 2]);
            const double cand_cost = red[nf * kBaRed];
            R.candidate_cost = cand_cost; R.model_change = model_change; R.step_norm = dn;
            R.status = tr_candidate(Q, &T, cand_cost, model_change, dn);
            if (R.status == VELO_BA_ACCEPTED) { st->cur = cand; R.status = tr_accept(Q, &T, sqrt(st->pose_xn2[cand] + red[nf * kBaRed + 3]), gradient_max(red)); }
        }
    }
    if (!T.done) tr_head(Q, &T);                                      // the head of the next iteration
    R.done = T.done; R.termination = T.termination; R.evaluations = T.evaluations; st->tr = T;
}
#else
;
#endif

}  // namespace velo
