// Driver of velo_hip::PoseGraph::covariance and jointCovariance (include/velo_pose_graph.hpp): reads a graph (poses by frame, edges, fixed
// frames and the two frames of a joint covariance), and prints every frame's marginal and the 12 x 12 as double bit patterns.  Without
// an argument it only has to compile and link -- with the call sites of before the covariance members too.
#include <cstdio>
#include <cstring>
#include <vector>

#include "velo_pose_graph.hpp"

static unsigned long long bits(double v) { unsigned long long u; std::memcpy(&u, &v, 8); return u; }

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

// the call sites that existed before still compile
int old_call_sites(velo_hip::PoseGraph& graph, const std::vector<int>& fixed, velo_graph_summary* s, const velo_graph_params* p) {
    return graph.optimize(fixed) | graph.optimize(fixed, s) | graph.optimize(fixed, s, p) | graph.optimize(fixed, s, p, VELO_GRAPH_SOLVER_ENVELOPE, 0);
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("pose graph covariance adaptor linked\n"); return 0; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int n_nodes = 0, n_edges = 0, n_fixed = 0, unused = 0, joint[2] = {0, 0};
    if (!rd(f, &n_nodes, 1) || !rd(f, &n_edges, 1) || !rd(f, &n_fixed, 1) || !rd(f, &unused, 1)) return 2;
    std::vector<int> frames(n_nodes), from(n_edges), to(n_edges), fixed(n_fixed);
    std::vector<double> poses(6 * (size_t)n_nodes), z(6 * (size_t)n_edges), info(n_edges);
    if (!rd(f, frames.data(), frames.size()) || !rd(f, poses.data(), poses.size()) || !rd(f, from.data(), from.size()) || !rd(f, to.data(), to.size()) ||
        !rd(f, z.data(), z.size()) || !rd(f, info.data(), info.size()) || !rd(f, fixed.data(), fixed.size()) || !rd(f, joint, 2)) return 2;
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
        // a refused call (a cap the graph exceeds) leaves the output alone
        std::vector<double> cov(1, 7.0);
        const int refused = graph.covariance(frames, fixed, &cov, 1) == VELO_ERR_INVALID && cov.size() == 1 && cov[0] == 7.0;
        if (graph.covariance(frames, fixed, &cov) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 5; }
        if (cov.size() != 36 * (size_t)n_nodes) return 5;
        for (int i = 0; i < n_nodes; i++) {
            printf("m %d", frames[i]);
            for (int j = 0; j < 36; j++) printf(" %016llx", bits(cov[36 * (size_t)i + j]));
            printf("\n");
        }
        double J[144];
        if (graph.jointCovariance(joint[0], joint[1], fixed, J) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 6; }
        printf("j %d %d", joint[0], joint[1]);
        for (int j = 0; j < 144; j++) printf(" %016llx", bits(J[j]));
        printf("\n");
        velo_hip::PoseGraph::Info info_out;
        graph.info(&info_out);
        printf("refused %d optimizations %d\n", refused ? 1 : 0, info_out.optimizations);
    }
    velo_destroy(ctx);
    return 0;
}
