// Driver of velo_hip::PoseGraph (include/velo_pose_graph.hpp): reads a graph (poses by frame, edges, fixed frames), optimises it and
// prints the summary and the poses as double bit patterns.  Edges with an even index go in as 6-vectors, the others as the 4 x 4 of
// velo_pose_vec_to_mat -- the caller's two forms.  Without an argument it only has to compile and link.
#include <cstdio>
#include <cstring>
#include <vector>

#include "velo_pose_graph.hpp"

static unsigned long long bits(double v) { unsigned long long u; std::memcpy(&u, &v, 8); return u; }

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

int main(int argc, char** argv) {
    if (argc < 2) { printf("pose graph adaptor linked\n"); return 0; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int n_nodes = 0, n_edges = 0, n_fixed = 0, as_matrix = 0;
    if (!rd(f, &n_nodes, 1) || !rd(f, &n_edges, 1) || !rd(f, &n_fixed, 1) || !rd(f, &as_matrix, 1)) return 2;
    std::vector<int> frames(n_nodes), from(n_edges), to(n_edges), fixed(n_fixed);
    std::vector<double> poses(6 * (size_t)n_nodes), z(6 * (size_t)n_edges), info(n_edges);
    if (!rd(f, frames.data(), frames.size()) || !rd(f, poses.data(), poses.size()) || !rd(f, from.data(), from.size()) || !rd(f, to.data(), to.size()) ||
        !rd(f, z.data(), z.size()) || !rd(f, info.data(), info.size()) || !rd(f, fixed.data(), fixed.size())) return 2;
    fclose(f);
    velo_ctx* ctx = 0;
    if (velo_create(&ctx, 0) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 3; }
    {
        velo_hip::PoseGraph graph(ctx);
        if (graph.status() != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 4; }
        for (int i = 0; i < n_nodes; i++)
            if (graph.setPose(frames[i], &poses[6 * (size_t)i]) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 4; }
        for (int e = 0; e < n_edges; e++) {
            int st;
            if (as_matrix && (e & 1)) {
                double Z[16];
                st = velo_pose_vec_to_mat(&z[6 * (size_t)e], Z);
                if (st == VELO_OK) st = graph.addEdgeMatrix(from[e], to[e], Z, info[e]);
            } else {
                st = graph.addEdge(from[e], to[e], &z[6 * (size_t)e], info[e]);
            }
            if (st != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 4; }
        }
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
        // a call the library refuses leaves the poses alone
        std::vector<double> kept, now;
        graph.poses(frames[0], 1, &kept);
        const int refused = graph.optimize(std::vector<int>()) == VELO_ERR_INVALID && graph.addEdge(frames[0], frames[0], &z[0], 1.0) == VELO_ERR_INVALID;
        graph.poses(frames[0], 1, &now);
        velo_hip::PoseGraph::Info info_out;
        graph.info(&info_out);
        printf("refused %d kept %d edges %d\n", refused ? 1 : 0, kept == now ? 1 : 0, info_out.edges);
    }
    velo_destroy(ctx);
    return 0;
}
