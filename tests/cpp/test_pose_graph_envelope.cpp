// Driver of velo_hip::PoseGraph::optimize with the envelope solver (include/velo_pose_graph.hpp): reads a graph (poses by frame, edges,
// fixed frames), optimises it with VELO_GRAPH_SOLVER_ENVELOPE and prints the summary, the poses as double bit patterns and the
// envelope's figures.  Without an argument it only has to compile and link -- with the call sites of before the solver argument too.
#include <cstdio>
#include <cstring>
#include <vector>

#include "velo_pose_graph.hpp"

static unsigned long long bits(double v) { unsigned long long u; std::memcpy(&u, &v, 8); return u; }

template <class T>
static bool rd(FILE* f, T* p, size_t n) { return n == 0 || fread(p, sizeof(T), n, f) == n; }

// the call sites that existed before the solver argument still compile, and mean the CG
int old_call_sites(velo_hip::PoseGraph& graph, const std::vector<int>& fixed, velo_graph_summary* s, const velo_graph_params* p) {
    return graph.optimize(fixed) | graph.optimize(fixed, s) | graph.optimize(fixed, s, p);
}

int main(int argc, char** argv) {
    if (argc < 2) { printf("pose graph envelope adaptor linked\n"); return 0; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) return 2;
    int n_nodes = 0, n_edges = 0, n_fixed = 0, unused = 0;
    if (!rd(f, &n_nodes, 1) || !rd(f, &n_edges, 1) || !rd(f, &n_fixed, 1) || !rd(f, &unused, 1)) return 2;
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
        for (int e = 0; e < n_edges; e++)
            if (graph.addEdge(from[e], to[e], &z[6 * (size_t)e], info[e]) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 4; }
        // refused calls leave the poses alone: a solver that does not exist, a cap the graph exceeds
        std::vector<double> kept, now;
        graph.poses(frames[n_nodes - 1], 1, &kept);
        const int refused = graph.optimize(fixed, 0, 0, 2) == VELO_ERR_INVALID && graph.optimize(fixed, 0, 0, VELO_GRAPH_SOLVER_ENVELOPE, 1) == VELO_ERR_INVALID;
        graph.poses(frames[n_nodes - 1], 1, &now);
        velo_graph_summary s;
        if (graph.optimize(fixed, &s, 0, VELO_GRAPH_SOLVER_ENVELOPE) != VELO_OK) { fprintf(stderr, "%s\n", velo_last_error()); return 5; }
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
        velo_hip::PoseGraph::Info info_out;
        graph.info(&info_out);
        printf("refused %d kept %d envelope %d %d\n", refused ? 1 : 0, kept == now ? 1 : 0, info_out.envelope_widest_row, info_out.envelope_blocks);
    }
    velo_destroy(ctx);
    return 0;
}
