// Driver of velo_hip::PoseGraph::retain, release and retained (include/velo_pose_graph.hpp): reads a graph that GROWS (every frame and
// every edge with the stage it arrives at), retains after stage 0, and after every stage prints the marginal of every posed frame and the
// relative covariance of (the second frame, the newest frame) as double bit patterns, then the retained state's counters.  Without an
// argument it only has to compile and link.
#include <cstdio>
#include <cstring>
#include <vector>

#include "velo_pose_graph.hpp"

static unsigned long long bits(double v) { unsigned long long u; std::memcpy(&u, &v, 8); return u; }

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

static void row(const char* tag, int s, int p, const double* v, int n) {
    printf("%s %d %d", tag, s, p);
    for (int j = 0; j < n; j++) printf(" %016llx", bits(v[j]));
    printf("\n");
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("pose graph retained adaptor linked\n"); return 0; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int n_nodes = 0, n_edges = 0, n_fixed = 0, n_stages = 0;
    if (!rd(f, &n_nodes, 1) || !rd(f, &n_edges, 1) || !rd(f, &n_fixed, 1) || !rd(f, &n_stages, 1)) return 2;
    std::vector<int> frames(n_nodes), frame_stage(n_nodes), from(n_edges), to(n_edges), edge_stage(n_edges), fixed(n_fixed);
    std::vector<double> poses(6 * (size_t)n_nodes), z(6 * (size_t)n_edges), info(n_edges);
    if (!rd(f, frames.data(), frames.size()) || !rd(f, frame_stage.data(), frame_stage.size()) || !rd(f, poses.data(), poses.size()) ||
        !rd(f, from.data(), from.size()) || !rd(f, to.data(), to.size()) || !rd(f, edge_stage.data(), edge_stage.size()) || !rd(f, z.data(), z.size()) ||
        !rd(f, info.data(), info.size()) || !rd(f, fixed.data(), fixed.size())) return 2;
    fclose(f);
    velo_ctx* ctx = 0;
    if (velo_create(&ctx, 0) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 3; }
    {
        velo_hip::PoseGraph graph(ctx);
        if (graph.status() != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 4; }
        std::vector<int> posed;
        for (int s = 0; s < n_stages; s++) {
            for (int i = 0; i < n_nodes; i++)
                if (frame_stage[i] == s) {
                    if (graph.setPose(frames[i], &poses[6 * (size_t)i]) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 4; }
                    posed.push_back(frames[i]);
                }
            for (int e = 0; e < n_edges; e++)
                if (edge_stage[e] == s && graph.addEdge(from[e], to[e], &z[6 * (size_t)e], info[e]) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 4; }
            if (s == 0 && graph.retain(fixed) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 5; }
            std::vector<double> cov, rel;
            if (graph.covariance(posed, fixed, &cov) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 6; }
            for (size_t p = 0; p < posed.size(); p++) row("cov", s, posed[p], &cov[36 * p], 36);
            const std::vector<int> a(1, posed[1]), b(1, posed.back());
            if (graph.relativeCovariance(a, b, fixed, &rel, &cov) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 7; }
            row("rel", s, posed.back(), &rel[0], 6);
            row("rcov", s, posed.back(), &cov[0], 36);
        }
        velo_hip::PoseGraph::Retained r;
        if (graph.retained(&r) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 8; }
        printf("retained state %d free %lld builds %lld extensions %lld rebuilds %lld served %lld perm", r.state, r.free_nodes, r.builds, r.extensions, r.rebuilds, r.served);
        for (size_t k = 0; k < r.perm.size(); k++) printf(" %d", r.perm[k]);
        printf("\n");
        if (graph.release() != VELO_OK || graph.retained(&r) != VELO_OK) return 9;
        printf("released state %d\n", r.state);
    }
    velo_destroy(ctx);
    return 0;
}
