// Driver of velo_hip::PoseGraph::gateEdges, relativeCovariance and loopCandidates (include/velo_pose_graph.hpp): reads a graph (poses by
// frame, edges, fixed frames) and the pairs to gate with their z and info21, and prints every pair's rel, r, S and chi2, the relative
// covariances and one candidate list as double bit patterns.  Without an argument it only has to compile and link.
#include <cstdio>
#include <cstring>
#include <vector>

#include "velo_pose_graph.hpp"

static unsigned long long bits(double v) { unsigned long long u; std::memcpy(&u, &v, 8); return u; }

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

static void row(const char* tag, int p, const double* v, int n) {
    printf("%s %d", tag, p);
    for (int j = 0; j < n; j++) printf(" %016llx", bits(v[j]));
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("pose graph gate adaptor linked\n"); return 0; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int n_nodes = 0, n_edges = 0, n_fixed = 0, n_pairs = 0, query[2] = {0, 0};
    if (!rd(f, &n_nodes, 1) || !rd(f, &n_edges, 1) || !rd(f, &n_fixed, 1) || !rd(f, &n_pairs, 1)) return 2;
    std::vector<int> frames(n_nodes), from(n_edges), to(n_edges), fixed(n_fixed), pa(n_pairs), pb(n_pairs);
    std::vector<double> poses(6 * (size_t)n_nodes), z(6 * (size_t)n_edges), info(n_edges), pz(6 * (size_t)n_pairs), pw(21 * (size_t)n_pairs);
    if (!rd(f, frames.data(), frames.size()) || !rd(f, poses.data(), poses.size()) || !rd(f, from.data(), from.size()) || !rd(f, to.data(), to.size()) ||
        !rd(f, z.data(), z.size()) || !rd(f, info.data(), info.size()) || !rd(f, fixed.data(), fixed.size()) || !rd(f, pa.data(), pa.size()) ||
        !rd(f, pb.data(), pb.size()) || !rd(f, pz.data(), pz.size()) || !rd(f, pw.data(), pw.size()) || !rd(f, query, 2)) return 2;
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
        // a refused call (a cap the graph exceeds) leaves the outputs alone
        std::vector<double> rel(1, 7.0), r(1, 7.0), cov(1, 7.0), chi2(1, 7.0);
        const int refused = graph.gateEdges(pa, pb, pz, pw, fixed, &rel, &r, &cov, &chi2, 1) == VELO_ERR_INVALID && rel.size() == 1 && rel[0] == 7.0 && chi2[0] == 7.0;
        if (graph.gateEdges(pa, pb, pz, pw, fixed, &rel, &r, &cov, &chi2) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 5; }
        if (rel.size() != 6 * (size_t)n_pairs || cov.size() != 36 * (size_t)n_pairs || chi2.size() != (size_t)n_pairs) return 5;
        for (int p = 0; p < n_pairs; p++) {
            row("rel", p, &rel[6 * (size_t)p], 6);
            row("r", p, &r[6 * (size_t)p], 6);
            row("S", p, &cov[36 * (size_t)p], 36);
            row("chi2", p, &chi2[(size_t)p], 1);
        }
        if (graph.relativeCovariance(pa, pb, fixed, &rel, &cov) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 6; }
        for (int p = 0; p < n_pairs; p++) { row("rrel", p, &rel[6 * (size_t)p], 6); row("rcov", p, &cov[36 * (size_t)p], 36); }
        std::vector<int> cand;
        std::vector<double> dist, sigma;
        if (graph.loopCandidates(query[0], query[1], 3.5, 2.0, fixed, &cand, &dist, &sigma, 1) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 7; }
        for (size_t k = 0; k < cand.size(); k++) { const double v[2] = {dist[k], sigma[k]}; row("cand", cand[k], v, 2); }
        velo_hip::PoseGraph::Info info_out;
        graph.info(&info_out);
        printf("refused %d optimizations %d\n", refused ? 1 : 0, info_out.optimizations);
    }
    velo_destroy(ctx);
    return 0;
}
