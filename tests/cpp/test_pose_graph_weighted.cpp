// Driver of velo_hip::PoseGraph's weighted members (include/velo_pose_graph.hpp): reads a graph (poses by frame, scalar edges, fixed
// frames, then registrations: ends, z, the registration's 6 x 6 and a loss scale), adds the scalar edges with addEdge and the
// registrations with addRegistration, optimises and prints the summary, the poses and edgeStats as double bit patterns.  Without an
// argument it only has to compile and link.
#include <cstdio>
#include <cstring>
#include <vector>

#include "velo_pose_graph.hpp"

static unsigned long long bits(double v) { unsigned long long u; std::memcpy(&u, &v, 8); return u; }

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

// every new member with its default argument, and addEdgeWeighted on its own
int call_sites(velo_hip::PoseGraph& graph, const double* z6, const double* info21, const double* JtJ36, std::vector<double>* out) {
    return graph.addEdgeWeighted(0, 1, z6, info21) | graph.addEdgeWeighted(0, 1, z6, info21, 2.0) | graph.addRegistration(0, 1, z6, JtJ36) |
           graph.addRegistration(0, 1, z6, JtJ36, 2.0) | graph.edgeStats(0, 1, out, out) | graph.edgeStats(0, 1, 0, 0);
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("pose graph weighted adaptor linked\n"); return 0; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int n_nodes = 0, n_edges = 0, n_fixed = 0, n_reg = 0;
    if (!rd(f, &n_nodes, 1) || !rd(f, &n_edges, 1) || !rd(f, &n_fixed, 1) || !rd(f, &n_reg, 1)) return 2;
    std::vector<int> frames(n_nodes), from(n_edges), to(n_edges), fixed(n_fixed), rfrom(n_reg), rto(n_reg);
    std::vector<double> poses(6 * (size_t)n_nodes), z(6 * (size_t)n_edges), info(n_edges), rz(6 * (size_t)n_reg), rH(36 * (size_t)n_reg), rloss(n_reg);
    if (!rd(f, frames.data(), frames.size()) || !rd(f, poses.data(), poses.size()) || !rd(f, from.data(), from.size()) || !rd(f, to.data(), to.size()) ||
        !rd(f, z.data(), z.size()) || !rd(f, info.data(), info.size()) || !rd(f, fixed.data(), fixed.size()) || !rd(f, rfrom.data(), rfrom.size()) ||
        !rd(f, rto.data(), rto.size()) || !rd(f, rz.data(), rz.size()) || !rd(f, rH.data(), rH.size()) || !rd(f, rloss.data(), rloss.size())) return 2;
    fclose(f);
    velo_ctx* ctx = 0;
    if (velo_create(&ctx, 0) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 3; }
    {
        velo_hip::PoseGraph graph(ctx);
        if (graph.status() != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 4; }
        for (int i = 0; i < n_nodes; i++)
            if (graph.setPose(frames[i], &poses[6 * (size_t)i]) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 4; }
        for (int e = 0; e < n_edges; e++)
            if (graph.addEdge(from[e], to[e], &z[6 * (size_t)e], info[e]) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 4; }
        for (int e = 0; e < n_reg; e++)
            if (graph.addRegistration(rfrom[e], rto[e], &rz[6 * (size_t)e], &rH[36 * (size_t)e], rloss[e]) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 4; }
        // a registration whose 6 x 6 is not positive definite is refused and leaves the edge count alone
        std::vector<double> neg(36, 0.0);
        for (int k = 0; k < 6; k++) neg[7 * (size_t)k] = -1.0;
        velo_hip::PoseGraph::Info before, after;
        graph.info(&before);
        const int refused = n_reg > 0 && graph.addRegistration(rfrom[0], rto[0], &rz[0], &neg[0]) == VELO_ERR_INVALID;
        graph.info(&after);
        velo_graph_summary s;
        if (graph.optimize(fixed, &s) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 5; }
        printf("s %d %d %d %d %d %d %d %016llx %016llx\n", s.termination, s.iterations, s.evaluations, s.n_nodes, s.n_free, s.n_edges, s.n_trace,
               bits(s.initial_cost), bits(s.final_cost));
        for (int k = 0; k < s.n_trace; k++)
            printf("t %d %d %d %016llx %016llx\n", s.trace[k].iteration, s.trace[k].status, s.trace[k].cg_iterations, bits(s.trace[k].cost), bits(s.trace[k].candidate_cost));
        for (int i = 0; i < n_nodes; i++) {
            std::vector<double> p;
            if (graph.poses(frames[i], 1, &p) != VELO_OK) return 6;
            printf("p %d", frames[i]);
            for (int j = 0; j < 6; j++) printf(" %016llx", bits(p[j]));
            printf("\n");
        }
        std::vector<double> chi2, weight;
        if (graph.edgeStats(0, n_edges + n_reg, &chi2, &weight) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 7; }
        for (size_t e = 0; e < chi2.size(); e++) printf("e %d %016llx %016llx\n", (int)e, bits(chi2[e]), bits(weight[e]));
        printf("refused %d kept %d\n", refused ? 1 : 0, before.edges == after.edges ? 1 : 0);
    }
    velo_destroy(ctx);
    return 0;
}
