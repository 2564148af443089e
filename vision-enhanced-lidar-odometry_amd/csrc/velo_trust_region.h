// velo_trust_region.h -- the trust-region Levenberg-Marquardt bookkeeping of SURVEY.md B1 (Ceres' defaults), once, for every solver that
// reduces an iteration to five numbers: candidate cost, model change, |step|, |x| and max |g|.  A solver owns its linear step and the
// decision whether that step is valid; the controller owns the rest.  Triangulation runs it per lane or wave (tri_solve,
// velo_tri_kernels.h: the shortest example of the calling sequence), bundle adjustment in one device thread (ba_decide_kernel), the pose
// graph on the host (velo_graph_optimize).  The scan-matching chain keeps its own fused transition (lm_transition_local, velo_kernels.h).
// Plain C++17, free of any HIP type: tests/cpp/test_trust_region.cpp runs it on its own against scripted solves.
#pragma once
#include <math.h>

#include "../../include/velo_hip.h"

#ifdef __HIPCC__
#define VELO_HD __host__ __device__
#else
#define VELO_HD
#endif

namespace velo {

struct LMParams {
    int max_num_iterations, max_invalid;
    double function_tolerance, gradient_tolerance, parameter_tolerance;
    double initial_radius, max_radius, min_radius, min_relative_decrease, min_diag, max_diag;
};

struct TrustRegion {
    double cost, x_norm;        // of the last accepted point
    double radius, decrease;    // mu and nu of B1
    double ratio;               // cost change / model change of the last candidate tr_candidate has seen
    int iteration, invalid;     // iterations begun; consecutive invalid steps
    int refresh;                // the next step recomputes the clipped diagonal D: at the start and after an accepted step
    int n_accepted, evaluations;
    int termination, done;      // VELO_CONVERGENCE / NO_CONVERGENCE / FAILURE (NO_CONVERGENCE while the solve runs); the solve has ended
};

// Every function returns the VELO_BA_* status of what it did, or whether the solve has ended.  A path that goes on writes its int fields
// BEFORE its doubles, so that only a path that ends the solve finishes with an int store: the device compiler merges sibling branches
// that finish with the same kind of store to different fields into one store through a selected address, and the state then leaves the
// registers (16 bytes of scratch in ba_decide_kernel and the triangulation kernels with `refresh` written last; tools/kernel_resources.py).

// after a rejected and after an invalid step; D is kept
VELO_HD inline void tr_shrink(TrustRegion* T) { T->refresh = 0; T->radius = T->radius / T->decrease; T->decrease *= 2.0; }
VELO_HD inline bool tr_stop(TrustRegion* T, int termination) { T->termination = termination; T->done = 1; return true; }

// the first evaluation: true when the gradient tolerance ends the solve there
VELO_HD inline bool tr_start(const LMParams& Q, TrustRegion* T, double cost, double x_norm, double max_gradient) {
    T->iteration = 0; T->invalid = 0; T->refresh = 1; T->n_accepted = 0; T->evaluations = 1; T->termination = VELO_NO_CONVERGENCE; T->done = 0;
    T->cost = cost; T->x_norm = x_norm; T->radius = Q.initial_radius; T->decrease = 2.0; T->ratio = 0.0;
    return max_gradient <= Q.gradient_tolerance && tr_stop(T, VELO_CONVERGENCE);
}

// the head of an iteration: true when the iteration limit or the smallest radius ends the solve, else the iteration has begun
VELO_HD inline bool tr_head(const LMParams& Q, TrustRegion* T) {
    if (T->iteration + 1 > Q.max_num_iterations) return tr_stop(T, VELO_NO_CONVERGENCE);
    if (T->radius < Q.min_radius) return tr_stop(T, VELO_CONVERGENCE);
    T->iteration++;
    return false;
}

// the linear solve failed or the model did not decrease: nothing was evaluated
VELO_HD inline int tr_invalid(const LMParams& Q, TrustRegion* T) {
    if (++T->invalid >= Q.max_invalid) tr_stop(T, VELO_FAILURE);
    else tr_shrink(T);
    return VELO_BA_INVALID;
}

// A valid step's candidate has been evaluated.  VELO_BA_PARAMETER / FUNCTION: the solve has ended where it stood.  VELO_BA_REJECTED: the
// radius has shrunk.  VELO_BA_ACCEPTED: the cost is the candidate's; the caller makes the candidate current and calls tr_accept.
VELO_HD inline int tr_candidate(const LMParams& Q, TrustRegion* T, double candidate_cost, double model_change, double step_norm) {
    T->invalid = 0; T->evaluations++;
    if (step_norm <= Q.parameter_tolerance * (T->x_norm + Q.parameter_tolerance)) { tr_stop(T, VELO_CONVERGENCE); return VELO_BA_PARAMETER; }
    const double cost_change = T->cost - candidate_cost;
    if (fabs(cost_change) <= Q.function_tolerance * T->cost) { tr_stop(T, VELO_CONVERGENCE); return VELO_BA_FUNCTION; }
    T->ratio = cost_change / model_change;
    if (!(T->ratio > Q.min_relative_decrease)) { tr_shrink(T); return VELO_BA_REJECTED; }
    T->n_accepted++; T->cost = candidate_cost;
    return VELO_BA_ACCEPTED;
}

// the accepted point's |x| and max |g|: VELO_BA_GRADIENT when the gradient tolerance ends the solve, else the radius grows and D is refreshed
VELO_HD inline int tr_accept(const LMParams& Q, TrustRegion* T, double x_norm, double max_gradient) {
    T->x_norm = x_norm;
    if (max_gradient <= Q.gradient_tolerance) { tr_stop(T, VELO_CONVERGENCE); return VELO_BA_GRADIENT; }
    const double t = 2.0 * T->ratio - 1.0;
    T->refresh = 1; T->decrease = 2.0;
    // (the division and the clamp, as two statements or as one expression, round the same: each operation is rounded on its own)
    T->radius = fmin(Q.max_radius, T->radius / fmax(1.0 / 3.0, 1.0 - t * t * t));
    return VELO_BA_ACCEPTED;
}

// ---- the packed upper triangle of a symmetric 6 x 6 block, row-major: 21 numbers ---------------------------------------------------
VELO_HD inline int upper6(int a, int b) { return a * 6 - (a * (a - 1)) / 2 + (b - a); }      // a <= b

// a 27-double record {upper 6 x 6 block, gradient (6)} to the gradient and the full block; either output may be null
inline void expand_upper6(const double* U, double* gradient, double* block) {
    for (int a = 0; a < 6; a++) {
        if (gradient) gradient[a] = U[21 + a];
        for (int b = 0; b < 6 && block; b++) block[6 * a + b] = U[a < b ? upper6(a, b) : upper6(b, a)];
    }
}

}  // namespace velo
