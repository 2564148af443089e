// velo_pose_graph.hpp -- header-only C++11 owner of a context's resident pose graph (velo_graph_*, include/velo_hip.h): one node per
// frame, one edge per accepted registration, and the batch optimisation that turns a loop closure into corrected poses -- what the
// reference's slam.add_node / add_factor / batch_optimization do (main.cpp:190-204, 516-536, 728-745).  Plain pointers and std::vector
// only; every member returns the C-ABI's status (VELO_OK == 0) and velo_last_error() has the text.
//
//     velo_hip::PoseGraph graph(ctx);
//     graph.setPose(frame, ceres_poses_vec[frame]);                 // a new node, or a node's new value
//     graph.addEdge(frame - dframe, frame, dpose16, 1.0);            // what frameToFrame returned, row-major 4 x 4 (or its 6-vector)
//     graph.addRegistration(loop_from, frame, z6, JtJ36, 2.0);       // a loop closure with velo_evaluate's 6 x 6 and Cauchy(2)
//     graph.optimize(fixed);                                         // fixed = {0}: the reference's prior on the first node
//     graph.optimize(fixed, &summary, 0, VELO_GRAPH_SOLVER_ENVELOPE); // the same with the exact envelope solver: a whole drive
//     graph.poses(0, n, &flat);                                      // n x 6, for velo_landmarks_set_pose / velo_map_set_pose
//     graph.covariance(frames, fixed, &cov36);                       // how well each pose is determined: 6 x 6 marginals
//     graph.jointCovariance(loop_from, frame, fixed, joint144);      // 12 x 12, the material of the gate below
//     graph.loopCandidates(frame, 50, 3.0, 3.0, fixed, &cand, 0, 0);  // frames within 3 m + 3 sigma of `frame`: what to try to close against
//     graph.gateEdges(from, to, z, info21, fixed, 0, 0, 0, &chi2);    // a proposed edge against the graph BEFORE it is added: chi2 with 6 dof
#ifndef VELO_POSE_GRAPH_HPP_
#define VELO_POSE_GRAPH_HPP_

#include <cstddef>
#include <vector>

#include "velo_hip.h"

namespace velo_hip {

class PoseGraph {
public:
    struct Info { int nodes, edges, edge_capacity, edge_reallocations, frame_capacity, optimizations, envelope_widest_row, envelope_blocks; };

    explicit PoseGraph(velo_ctx* ctx, int edge_capacity = 0) : ctx_(ctx), status_(velo_graph_reset(ctx, edge_capacity)) {}

    int status() const { return status_; }                 // of the constructor's velo_graph_reset

    int setPose(int frame, const double pose6[6]) { return velo_graph_set_pose(ctx_, frame, pose6); }
    int setPoses(int first, const std::vector<double>& flat) { return velo_graph_set_poses(ctx_, first, (int32_t)(flat.size() / 6), flat.empty() ? 0 : &flat[0]); }

    // pose_to = pose_from . Z: Z as its 6-vector (angle-axis, translation) ...
    int addEdge(int from, int to, const double z6[6], double info) {
        const int32_t a = from, b = to;
        return velo_graph_add_edges(ctx_, 1, &a, &b, z6, &info);
    }
    // ... or as a row-major 4 x 4 (Eigen::Matrix4d is column-major: pass its transpose's data, or fill the 16 doubles by (row, col))
    int addEdgeMatrix(int from, int to, const double Z16[16], double info) {
        double z6[6];
        const int st = velo_pose_mat_to_vec(Z16, z6);
        return st != VELO_OK ? st : addEdge(from, to, z6, info);
    }
    // many at once: z holds 6 doubles per edge
    int addEdges(const std::vector<int>& from, const std::vector<int>& to, const std::vector<double>& z, const std::vector<double>& info) {
        if (from.size() != to.size() || z.size() != 6 * from.size() || info.size() != from.size()) return VELO_ERR_INVALID;
        if (from.empty()) return VELO_OK;
        std::vector<int32_t> a(from.begin(), from.end()), b(to.begin(), to.end());
        return velo_graph_add_edges(ctx_, (int32_t)a.size(), &a[0], &b[0], &z[0], &info[0]);
    }

    // an edge with a 6 x 6 information (info21: W's upper triangle, row by row) and a loss: 0 = trivial, a > 0 = Cauchy(a) on r^T W r
    int addEdgeWeighted(int from, int to, const double z6[6], const double info21[21], double loss_scale = 0.0) {
        const int32_t a = from, b = to;
        return velo_graph_add_edges_weighted(ctx_, 1, &a, &b, z6, info21, &loss_scale);
    }
    // a registration as an edge: z6 its result, JtJ36 its 6 x 6 at that result as velo_evaluate returns it (velo_graph_edge_information)
    int addRegistration(int from, int to, const double z6[6], const double JtJ36[36], double loss_scale = 0.0) {
        double info21[21];
        const int st = velo_graph_edge_information(z6, JtJ36, info21);
        return st != VELO_OK ? st : addEdgeWeighted(from, to, z6, info21, loss_scale);
    }
    // chi2 = r^T W r and weight = rho'(chi2) of the edges first .. first + n - 1 at the stored poses, in the order they were added
    int edgeStats(int first, int n, std::vector<double>* chi2, std::vector<double>* weight) const {
        std::vector<double> s((size_t)(n > 0 ? n : 0) + 1), w(s.size());
        const int st = velo_graph_edge_stats(ctx_, first, n, &s[0], &w[0]);
        if (st != VELO_OK) return st;
        s.resize((size_t)n); w.resize((size_t)n);
        if (chi2) chi2->swap(s);
        if (weight) weight->swap(w);
        return VELO_OK;
    }

    // refines every node that has a pose and is not in `fixed` (ascending frame numbers).  solver: VELO_GRAPH_SOLVER_CG (what params
    // say, or the defaults) or VELO_GRAPH_SOLVER_ENVELOPE, the exact envelope Cholesky that carries a whole drive; max_work: its cap in
    // block products per factorisation (0: the library's default) -- a graph over it is refused and nothing changes
    int optimize(const std::vector<int>& fixed, velo_graph_summary* summary = 0, const velo_graph_params* params = 0,
                 int solver = VELO_GRAPH_SOLVER_CG, int max_work = 0) {
        std::vector<int32_t> f(fixed.begin(), fixed.end());
        velo_graph_params own;
        if (solver != VELO_GRAPH_SOLVER_CG || max_work != 0) {
            if (params) own = *params;
            else { const int st = velo_default_graph_params(&own); if (st != VELO_OK) return st; }
            own.reserved[0] = solver; own.reserved[1] = max_work;
            params = &own;
        }
        return velo_graph_optimize(ctx_, f.empty() ? 0 : &f[0], (int32_t)f.size(), params, summary);
    }

    // the nodes first .. first + n - 1, 6 doubles each
    int poses(int first, int n, std::vector<double>* flat) const {
        std::vector<double> out(6 * (size_t)(n > 0 ? n : 0) + 6);
        const int st = velo_graph_get_poses(ctx_, first, n, &out[0]);
        if (st != VELO_OK) return st;
        out.resize(6 * (size_t)n);
        flat->swap(out);
        return VELO_OK;
    }
    // the marginal covariance of every frame of `frames` at the stored poses (velo_graph_covariance): 36 doubles each, row-major, in the
    // coordinates of a node's 6 doubles; zeros for a fixed frame.  fixed: as for optimize; max_work: the envelope's cap (0: the default)
    int covariance(const std::vector<int>& frames, const std::vector<int>& fixed, std::vector<double>* cov36, int max_work = 0) const {
        std::vector<int32_t> a(frames.begin(), frames.end());
        return covariancePairs(a, a, fixed, cov36, max_work);
    }
    // the 12 x 12 joint covariance of frames a and b, row-major, from the three blocks of one call: [Saa Sab; Sab^T Sbb]
    int jointCovariance(int a, int b, const std::vector<int>& fixed, double joint144[144], int max_work = 0) const {
        std::vector<int32_t> fa(3, (int32_t)a), fb(3, (int32_t)b);
        fb[0] = a; fa[2] = b;                                          // (a, a), (a, b), (b, b)
        std::vector<double> blk;
        const int st = covariancePairs(fa, fb, fixed, &blk, max_work);
        if (st != VELO_OK) return st;
        for (int r = 0; r < 6; r++)
            for (int c = 0; c < 6; c++) {
                joint144[r * 12 + c] = blk[(size_t)(r * 6 + c)];
                joint144[r * 12 + 6 + c] = blk[(size_t)(36 + r * 6 + c)];
                joint144[(6 + c) * 12 + r] = blk[(size_t)(36 + r * 6 + c)];
                joint144[(6 + r) * 12 + 6 + c] = blk[(size_t)(72 + r * 6 + c)];
            }
        return VELO_OK;
    }

    // proposed edges tested against the graph BEFORE they enter it (velo_graph_edge_gate), at the stored poses -- optimise first.  z: 6
    // doubles per pair, or empty (every pair's own stored relative pose); info21: 21 per pair, or empty (S = Sigma_rel).  Per pair:
    // rel6 (6), r6 (6), cov36 = Sigma_rel + W^-1 (36), chi2 = r^T S^-1 r (-1 where S is not positive definite), to be compared with a
    // chi-square quantile of 6 degrees of freedom.  Every output may be null.
    int gateEdges(const std::vector<int>& from, const std::vector<int>& to, const std::vector<double>& z, const std::vector<double>& info21,
                  const std::vector<int>& fixed, std::vector<double>* rel6, std::vector<double>* r6, std::vector<double>* cov36, std::vector<double>* chi2,
                  int max_work = 0) const {
        const size_t n = from.size();
        if (to.size() != n || (!z.empty() && z.size() != 6 * n) || (!info21.empty() && info21.size() != 21 * n)) return VELO_ERR_INVALID;
        std::vector<int32_t> a(from.begin(), from.end()), b(to.begin(), to.end()), f(fixed.begin(), fixed.end());
        velo_graph_params own;
        const int ps = velo_default_graph_params(&own);
        if (ps != VELO_OK) return ps;
        own.reserved[1] = max_work;
        std::vector<double> rel(6 * n + 6), r(6 * n + 6), cov(36 * n + 36), c2(n + 1);
        const int st = velo_graph_edge_gate(ctx_, f.empty() ? 0 : &f[0], (int32_t)f.size(), &own, (int32_t)n, n ? &a[0] : 0, n ? &b[0] : 0,
                                            z.empty() ? 0 : &z[0], info21.empty() ? 0 : &info21[0], &rel[0], &r[0], &cov[0], &c2[0]);
        if (st != VELO_OK) return st;
        rel.resize(6 * n); r.resize(6 * n); cov.resize(36 * n); c2.resize(n);
        if (rel6) rel6->swap(rel);
        if (r6) r6->swap(r);
        if (cov36) cov36->swap(cov);
        if (chi2) chi2->swap(c2);
        return VELO_OK;
    }
    // the stored relative pose of every pair (a, b) and its covariance in the tangent at that pose: gateEdges without a measurement and
    // without an information.  Unlike the marginals it does not depend on which frame is fixed.
    int relativeCovariance(const std::vector<int>& a, const std::vector<int>& b, const std::vector<int>& fixed, std::vector<double>* rel6,
                           std::vector<double>* cov36, int max_work = 0) const {
        return gateEdges(a, b, std::vector<double>(), std::vector<double>(), fixed, rel6, 0, cov36, 0, max_work);
    }
    // loop-closure candidates of `query` (velo_graph_loop_candidates): the frames i with |i - query| >= min_gap whose stored distance to
    // the query is at most radius + k_sigma . sigma_i, ascending, with that distance and sigma_i (0 for k_sigma == 0, which runs no
    // factorisation); asks again when the first room was too small -- a second whole call, factorisation included, so where more than
    // `capacity` candidates can be expected (a long drive, a wide radius) give the room at once.  max_work: the envelope's cap (0: the
    // default).  Every output may be null.
    int loopCandidates(int query, int min_gap, double radius, double k_sigma, const std::vector<int>& fixed, std::vector<int>* frames,
                       std::vector<double>* dist, std::vector<double>* sigma, int capacity = 64, int max_work = 0) const {
        std::vector<int32_t> f(fixed.begin(), fixed.end());
        velo_graph_params own;
        const int ps = velo_default_graph_params(&own);
        if (ps != VELO_OK) return ps;
        own.reserved[1] = max_work;
        int32_t cap = capacity > 0 ? capacity : 1;
        for (;;) {
            std::vector<int32_t> fr((size_t)cap);
            std::vector<double> d((size_t)cap), s((size_t)cap);
            int32_t found = 0;
            const int st = velo_graph_loop_candidates(ctx_, f.empty() ? 0 : &f[0], (int32_t)f.size(), &own, query, min_gap, radius, k_sigma, cap, &fr[0], &d[0], &s[0], &found);
            if (st != VELO_OK) return st;
            if (found > cap) { cap = found; continue; }
            d.resize((size_t)found); s.resize((size_t)found);
            if (frames) frames->assign(fr.begin(), fr.begin() + found);
            if (dist) dist->swap(d);
            if (sigma) sigma->swap(s);
            return VELO_OK;
        }
    }

    // Keeps the factorisation covariance, gateEdges and loopCandidates (k_sigma > 0) build for this `fixed` set (velo_graph_retain), so that
    // they stop building it per call; setPose of a NEW frame above every retained free one and addEdge leave it behind, and the next query
    // extends it from the first row they touch.  perm: the order of the free nodes' indices to factor in, or empty (frame order, unless
    // that costs more than VELO_GRAPH_RETAIN_REBUILD_RATIO times velo_graph_order's).  optimize drops it: retain again after a solve.
    int retain(const std::vector<int>& fixed, const std::vector<int>& perm = std::vector<int>(), int max_work = 0) {
        std::vector<int32_t> f(fixed.begin(), fixed.end()), p(perm.begin(), perm.end());
        velo_graph_params own;
        const int ps = velo_default_graph_params(&own);
        if (ps != VELO_OK) return ps;
        own.reserved[1] = max_work;
        return velo_graph_retain(ctx_, f.empty() ? 0 : &f[0], (int32_t)f.size(), &own, p.empty() ? 0 : &p[0], (int32_t)p.size());
    }
    int release() { return velo_graph_release(ctx_); }
    struct Retained {
        int state;                                         // 0 none, 1 current, 2 behind
        long long free_nodes, widest_row, blocks, work, builds, extensions, rebuilds, selected_inverses, columns, served, first_dirty_row, rows_refactored;
        std::vector<int> perm;                             // the retained order: free indices by position
    };
    int retained(Retained* out) const {
        int64_t v[16];
        int st = velo_graph_retained(ctx_, v, 0, 0);
        if (st != VELO_OK) return st;
        std::vector<int32_t> p((size_t)v[1] + 1);
        st = velo_graph_retained(ctx_, v, &p[0], (int32_t)v[1]);
        if (st != VELO_OK) return st;
        out->state = (int)v[0]; out->free_nodes = v[1]; out->widest_row = v[2]; out->blocks = v[3]; out->work = v[4]; out->builds = v[5];
        out->extensions = v[6]; out->rebuilds = v[7]; out->selected_inverses = v[8]; out->columns = v[9]; out->served = v[10];
        out->first_dirty_row = v[11]; out->rows_refactored = v[12];
        out->perm.assign(p.begin(), p.begin() + (size_t)v[1]);
        return VELO_OK;
    }

    int info(Info* out) const {
        int32_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const int st = velo_graph_info(ctx_, v);
        out->nodes = v[0]; out->edges = v[1]; out->edge_capacity = v[2]; out->edge_reallocations = v[3]; out->frame_capacity = v[4];
        out->optimizations = v[5]; out->envelope_widest_row = v[6]; out->envelope_blocks = v[7];
        return st;
    }

private:
    int covariancePairs(const std::vector<int32_t>& a, const std::vector<int32_t>& b, const std::vector<int>& fixed, std::vector<double>* cov36, int max_work) const {
        std::vector<int32_t> f(fixed.begin(), fixed.end());
        velo_graph_params own;
        const int ps = velo_default_graph_params(&own);
        if (ps != VELO_OK) return ps;
        own.reserved[1] = max_work;
        std::vector<double> out(36 * a.size() + 36);
        const int st = velo_graph_covariance(ctx_, f.empty() ? 0 : &f[0], (int32_t)f.size(), &own, (int32_t)a.size(), a.empty() ? 0 : &a[0], b.empty() ? 0 : &b[0], &out[0]);
        if (st != VELO_OK) return st;
        out.resize(36 * a.size());
        cov36->swap(out);
        return VELO_OK;
    }
    PoseGraph(const PoseGraph&);                           // one owner of the context's store
    PoseGraph& operator=(const PoseGraph&);
    velo_ctx* ctx_;
    int status_;
};

}  // namespace velo_hip

#endif  // VELO_POSE_GRAPH_HPP_
