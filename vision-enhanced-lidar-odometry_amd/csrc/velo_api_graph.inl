// velo_api_graph.inl -- part of the host side of the C-ABI, included by velo_hip.hip (ONE translation unit; the order of the parts is the order of
// definition).  C-ABI: the resident pose graph of a drive and its batch optimisation (velo_graph_*); the kernels and the scheme of one
// LM iteration are in velo_graph_kernels.h.
//
// Who knows what: the DEVICE holds the edges (from, to, z, info; appended, never sent again) and every block the solver forms from them.
// The HOST keeps the ints of the edges -- enough to refuse a call and to build the incidence lists -- and a pinned mirror of the poses:
// a pose arrives from the host (velo_graph_set_pose) and leaves to it (velo_graph_get_poses), so the mirror is the one copy both
// directions share, and a solve starts by sending it.  The LM decision is taken here, from one GraphRecord per iteration.
// velo_graph_retain: the factorisation of velo_graph_covariance's problem, kept between calls.  It owns every buffer a query on it reads
// -- the order's ints, the skyline of L, the Jacobi scales, the poses it was linearised at, the skyline of Z, the full columns -- so a
// call that does not use it cannot disturb it; the work buffers of a build or an extension (graph_begin's) are the store's.
struct GraphRetained {
    int state = 0;                                       // 0 none, 1 current, 2 behind (the store has been appended to since)
    std::vector<int32_t> fixed, free_nodes;
    std::vector<int32_t> ints;                           // of the generation: perm [n], pos [n], first [n], rowptr [n + 1], last [n]
    int64_t max_work = 0, stats[4] = {0, 0, 0, 0};       // the cap it was retained under; widest row, blocks, work, components
    size_t edges_seen = 0, frames = 0;                   // the store's edges the generation covers; the node table's rows in x
    int valid_rows = 0;                                  // the device rows < valid_rows hold the generation's L (less than n after an extension failed)
    bool z_valid = false;                                // zenv holds the generation's selected inverse
    int col_pos = -1;                                    // the position whose full column slot 0 of `col` holds; -1: none
    int64_t counters[6] = {0, 0, 0, 0, 0, 0};            // full builds, extensions, rebuilds, selected inverses, full columns, queries served
    int64_t last_p = 0, last_rows = 0;                   // of the last extension: its first dirty row, the rows it refactored
    DevBuf<int> idx;
    DevBuf<double> env, zenv, scale, x, col;
    PinBuf<> h_idx;
};

struct GraphStore {
    GraphRetained ret;
    // device: the edges
    DevBuf<int> from, to;
    DevBuf<double> z, info;
    // a store that has seen velo_graph_add_edges_weighted: per edge the Cholesky factor of its 6 x 6 information (21 doubles) and its loss
    // scale; a scalar edge is info . I with the trivial loss there (graph_promote_kernel), and `info` is no longer read for any edge
    DevBuf<double> winfo, wloss, estat;
    bool weighted = false;
    size_t n_edges = 0, edge_cap = 0;
    int edge_reallocs = 0, n_optimized = 0;
    // the nodes: [2][frame_cap][6] on the device (current / candidate), [frame_cap][6] pinned
    DevBuf<double> x;
    PinBuf<double> h_x;
    size_t frame_cap = 0;
    std::vector<unsigned char> pose_set;
    int n_nodes = 0;
    // host: ints only
    std::vector<int32_t> h_from, h_to;
    // staging (an upload is followed by an event; a solve ends with a synchronisation) and the work buffers of a solve
    PinBuf<> h_in, h_st, h_out;
    Event in_ev;
    DevBuf<int> node, inc_start, inc;
    DevBuf<double> blk, nd, vec, part, nterm;
    DevBuf<GraphRecord> rec;
    // the envelope solver: the order's ints (perm, pos, first, rowptr, last) and the block skyline, which keeps its size between calls
    DevBuf<int> env_idx;
    DevBuf<double> env;
    int env_widest = 0, env_blocks = 0;                  // of the last envelope solve (velo_graph_info)
    // velo_graph_covariance: the selected inverse (a second skyline), the column solves' work vectors, the pairs' ints, and the record
    // with the pairs' blocks behind it (one copy to the host)
    DevBuf<double> cov_z, cov_work, cov_out;
    DevBuf<int> cov_pair;
    // velo_graph_edge_gate, velo_graph_loop_candidates: the pairs' (the frames') ints and doubles; the factor, the selected inverse, the
    // work vectors and the record are the covariance's
    DevBuf<double> rel_d;
    DevBuf<int> rel_i;
};

namespace {

constexpr size_t kGraphDefaultEdges = 4096;
constexpr int kGraphVec = 6 + 6 + 21 + 4 * 6 + 2 * 6;      // per free node: scale, diag, chol, y, r, z, q, p[2]

int graph_need_store(velo_ctx* c, const char* who) {
    if (!c->graph) return fail(VELO_ERR_STATE, "%s: velo_graph_reset has not run on this context", who);
    return VELO_OK;
}

velo_graph_params graph_params(const velo_graph_params* params) {     // a call's own, or the defaults
    velo_graph_params p;
    velo_default_graph_params(&p);
    return params ? *params : p;
}

int64_t graph_work_cap(const velo_graph_params* params) {            // a call's cap on the envelope solver's work
    return params && params->reserved[1] > 0 ? params->reserved[1] : VELO_GRAPH_DEFAULT_MAX_WORK;
}

bool graph_has_pose(const GraphStore& S, int64_t frame) { return (size_t)frame < S.pose_set.size() && S.pose_set[(size_t)frame]; }

struct GraphCall {
    GraphArgs A;
    GraphWeights W = {nullptr, nullptr, nullptr};        // of a weighted store
    std::vector<int32_t> free_nodes;
    int n_free = 0, E = 0;
    bool envelope = false;                               // set by the caller: graph_begin then orders the free nodes and checks the work
    int64_t max_work = 0, env_stats[4] = {0, 0, 0, 0};
    const char* who = "velo_graph_optimize";             // the entry a refusal names
    std::vector<int32_t> env_ints;                       // of an envelope call: perm [n], pos [n], first [n], rowptr [n + 1], last [n]
};

// What moves a retained factorisation on (include/velo_hip.h, velo_graph_retain): an append leaves it behind, everything else drops it.
// The buffers and the counters stay with the store.
void graph_ret_drop(GraphStore& S) { S.ret.state = 0; S.ret.z_valid = false; S.ret.col_pos = -1; S.ret.valid_rows = 0; }
void graph_ret_behind(GraphStore& S) { if (S.ret.state == 1) S.ret.state = 2; }

// an order's ints as the kernels take them: perm [n], pos [n], first [n], rowptr [n + 1], last [n]
void graph_env_ints(size_t n, const int32_t* perm, const int32_t* first, std::vector<int32_t>* out) {
    out->resize(5 * n + 1);
    int32_t* pos = out->data() + n;
    int32_t* rowptr = out->data() + 3 * n;
    int32_t* last = out->data() + 4 * n + 1;
    std::memcpy(out->data(), perm, sizeof(int32_t) * n);
    std::memcpy(out->data() + 2 * n, first, sizeof(int32_t) * n);
    rowptr[0] = 0;
    for (size_t k = 0; k < n; k++) { pos[(size_t)perm[k]] = (int32_t)k; rowptr[k + 1] = rowptr[k] + ((int32_t)k - first[k] + 1); last[k] = (int32_t)k; }
    for (size_t k = 0; k < n; k++) last[(size_t)first[k]] = std::max(last[(size_t)first[k]], (int32_t)k);
    for (size_t k = 1; k < n; k++) last[k] = std::max(last[k], last[k - 1]);      // the last row whose first column is <= k
}

// that layout on the device, and the skyline it indexes, as a kernel's arguments
void graph_env_bind(GraphArgs* A, const int* idx, size_t n, double* env) {
    A->env_perm = idx; A->env_pos = idx + n; A->env_first = idx + 2 * n; A->env_rowptr = idx + 3 * n; A->env_last = idx + 4 * n + 1;
    A->env = env;
}

// what an order may not exceed, refused before anything is sent; advice: what the entry's caller can do about the cap
int graph_env_refusal(const char* who, const int64_t* stats, int64_t max_work, size_t n, const char* advice) {
    if (stats[2] > max_work)
        return fail(VELO_ERR_INVALID, "%s: the envelope solver's work is %lld block products, over the cap of %lld (widest row %lld blocks, %lld free nodes); %s",
                    who, (long long)stats[2], (long long)max_work, (long long)stats[0], (long long)n, advice);
    if (stats[1] > (int64_t)1 << 30) return fail(VELO_ERR_INVALID, "%s: an envelope of %lld blocks; at most 2^30", who, (long long)stats[1]);
    return VELO_OK;
}

// velo_graph_order's rule (include/velo_hip.h), on checked arguments
void graph_order(int32_t n, int32_t m, const int32_t* ea, const int32_t* eb, int32_t* perm, int32_t* first, int64_t* stats) {
    const size_t N = (size_t)n;
    std::vector<int32_t> start(N + 1, 0), adj;
    for (int32_t e = 0; e < m; e++) { start[(size_t)ea[e] + 1]++; start[(size_t)eb[e] + 1]++; }
    for (size_t i = 0; i < N; i++) start[i + 1] += start[i];
    adj.resize((size_t)start[N]);
    {
        std::vector<int32_t> fill(start.begin(), start.end() - 1);
        for (int32_t e = 0; e < m; e++) { adj[(size_t)fill[(size_t)ea[e]]++] = eb[e]; adj[(size_t)fill[(size_t)eb[e]]++] = ea[e]; }
    }
    std::vector<int32_t> deg(N, 0);
    for (size_t i = 0; i < N; i++) {                                   // distinct neighbours, ascending, at the front of the node's list
        int32_t* lo = adj.data() + start[i];
        int32_t* hi = adj.data() + start[i + 1];
        std::sort(lo, hi);
        deg[i] = (int32_t)(std::unique(lo, hi) - lo);
    }
    auto less = [&](int32_t u, int32_t v) { return deg[(size_t)u] != deg[(size_t)v] ? deg[(size_t)u] < deg[(size_t)v] : u < v; };
    std::vector<int32_t> seen(N, -1), queue(N), level(N, 0), order;
    std::vector<unsigned char> placed(N, 0);
    order.reserve(N);
    int32_t stamp = 0;
    // the breadth-first level structure rooted at r: the number of levels; queue[0 .. count) holds the component by level
    auto levels = [&](int32_t r, size_t* count, size_t* last_begin) {
        seen[(size_t)r] = ++stamp;
        level[(size_t)r] = 0;
        queue[0] = r;
        size_t head = 0, tail = 1, lb = 0;
        while (head < tail) {
            const int32_t u = queue[head++];
            if (level[(size_t)u] > level[(size_t)queue[lb]]) lb = head - 1;
            for (int32_t k = 0; k < deg[(size_t)u]; k++) {
                const int32_t v = adj[(size_t)start[(size_t)u] + (size_t)k];
                if (seen[(size_t)v] != stamp) { seen[(size_t)v] = stamp; level[(size_t)v] = level[(size_t)u] + 1; queue[tail++] = v; }
            }
        }
        *count = tail; *last_begin = lb;
        return level[(size_t)queue[tail - 1]] + 1;
    };
    int64_t components = 0;
    std::vector<int32_t> nb;
    for (int32_t s = 0; s < n; s++) {
        if (placed[(size_t)s]) continue;
        components++;
        size_t count = 0, lb = 0;
        levels(s, &count, &lb);
        int32_t root = queue[0];
        for (size_t k = 1; k < count; k++) if (less(queue[k], root)) root = queue[k];
        int32_t height = levels(root, &count, &lb);
        for (;;) {
            int32_t far = queue[lb];
            for (size_t k = lb + 1; k < count; k++) if (less(queue[k], far)) far = queue[k];
            const int32_t h = levels(far, &count, &lb);
            if (h <= height) break;
            root = far; height = h;
        }
        const size_t base = order.size();                              // Cuthill-McKee from the root; `order` is its own queue
        order.push_back(root);
        placed[(size_t)root] = 1;
        for (size_t head = base; head < order.size(); head++) {
            const int32_t u = order[head];
            nb.clear();
            for (int32_t k = 0; k < deg[(size_t)u]; k++) {
                const int32_t v = adj[(size_t)start[(size_t)u] + (size_t)k];
                if (!placed[(size_t)v]) { placed[(size_t)v] = 1; nb.push_back(v); }
            }
            std::sort(nb.begin(), nb.end(), less);
            order.insert(order.end(), nb.begin(), nb.end());
        }
    }
    std::vector<int32_t> pos(N);
    for (size_t k = 0; k < N; k++) { perm[k] = order[N - 1 - k]; pos[(size_t)perm[k]] = (int32_t)k; }
    int64_t widest = 0, blocks = 0, work = 0;
    for (size_t k = 0; k < N; k++) {
        const size_t u = (size_t)perm[k];
        int32_t f = (int32_t)k;
        for (int32_t q = 0; q < deg[u]; q++) f = std::min(f, pos[(size_t)adj[(size_t)start[u] + (size_t)q]]);
        first[k] = f;
        const int64_t w = (int64_t)k - f;
        widest = std::max(widest, w); blocks += w + 1; work += w * (w + 1) / 2;
    }
    stats[0] = widest; stats[1] = blocks; stats[2] = work; stats[3] = components;
}

// first[k] = the smallest position among k and the neighbours of perm[k], by definition, over the edges [0, m); widest row, blocks, work
void graph_first_of(int32_t n, int32_t m, const int32_t* ea, const int32_t* eb, const int32_t* perm, int32_t* first, int64_t* stats3) {
    std::vector<int32_t> pos((size_t)n);
    for (int32_t k = 0; k < n; k++) { pos[(size_t)perm[k]] = k; first[k] = k; }
    for (int32_t e = 0; e < m; e++) {
        const int32_t pa = pos[(size_t)ea[e]], pb = pos[(size_t)eb[e]];
        first[std::max(pa, pb)] = std::min(first[std::max(pa, pb)], std::min(pa, pb));
    }
    int64_t widest = 0, blocks = 0, work = 0;
    for (int32_t k = 0; k < n; k++) {
        const int64_t w = (int64_t)k - first[k];
        widest = std::max(widest, w); blocks += w + 1; work += w * (w + 1) / 2;
    }
    stats3[0] = widest; stats3[1] = blocks; stats3[2] = work;
}

// velo_graph_order_extend's rule (include/velo_hip.h), on checked arguments (perm_old a permutation, the old edges among the old nodes).
// False when a row before the first dirty one does not keep its `first`: cannot happen, and is checked.
bool graph_order_extend(int32_t n_old, const int32_t* perm_old, int32_t n, int32_t m, const int32_t* ea, const int32_t* eb, int32_t first_new,
                        int64_t max_work, int32_t* perm, int32_t* first, int64_t* stats) {
    const size_t N = (size_t)n;
    // the fresh order, oriented
    std::vector<int32_t> fperm(N), ffirst(N);
    int64_t fs[4] = {0, 0, 0, 0};
    graph_order(n, m, ea, eb, fperm.data(), ffirst.data(), fs);
    bool reversed = false;
    if (n > 0) {
        int32_t at = 0;
        for (int32_t k = 0; k < n; k++) if (fperm[(size_t)k] == n - 1) at = k;
        if (2 * (int64_t)at < n && 2 * (int64_t)(n - 1 - at) >= n) {
            std::vector<int32_t> rperm(fperm.rbegin(), fperm.rend()), rfirst(N);
            int64_t rs[3];
            graph_first_of(n, m, ea, eb, rperm.data(), rfirst.data(), rs);
            if (rs[2] <= (int64_t)VELO_GRAPH_RETAIN_REBUILD_RATIO * fs[2]) {
                reversed = true;
                fperm.swap(rperm); ffirst.swap(rfirst);
                fs[0] = rs[0]; fs[1] = rs[1]; fs[2] = rs[2];
            }
        }
    }
    // the extended order and its first dirty row
    std::vector<int32_t> pos(N), old_first((size_t)n_old);
    for (int32_t k = 0; k < n; k++) { perm[k] = k < n_old ? perm_old[k] : k; pos[(size_t)perm[k]] = k; }
    int32_t p = n_old < n ? n_old : n;
    for (int32_t e = first_new; e < m; e++) p = std::min(p, std::min(pos[(size_t)ea[e]], pos[(size_t)eb[e]]));
    int64_t os[3], es[3];
    if (n_old > 0) graph_first_of(n_old, first_new, ea, eb, perm_old, old_first.data(), os);
    graph_first_of(n, m, ea, eb, perm, first, es);
    for (int32_t k = 0; k < std::min(p, n_old); k++) if (first[k] != old_first[(size_t)k]) return false;
    const bool keep = es[2] <= max_work && es[2] <= (int64_t)VELO_GRAPH_RETAIN_REBUILD_RATIO * fs[2];
    if (keep) { stats[0] = es[0]; stats[1] = es[1]; stats[2] = es[2]; }
    else {
        std::memcpy(perm, fperm.data(), sizeof(int32_t) * N);
        std::memcpy(first, ffirst.data(), sizeof(int32_t) * N);
        stats[0] = fs[0]; stats[1] = fs[1]; stats[2] = fs[2];
        p = 0;
    }
    stats[3] = fs[3]; stats[4] = p; stats[5] = keep ? 0 : 1; stats[6] = !keep && reversed ? 1 : 0; stats[7] = fs[2];
    return true;
}

int graph_check(velo_ctx* c, const int32_t* fixed, int32_t n_fixed, const velo_graph_params* params, const char* who) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    if (n_fixed < 1) return fail(VELO_ERR_INVALID, "%s: %d fixed nodes; at least 1 fixes the gauge", who, n_fixed);
    if (!fixed) return fail(VELO_ERR_INVALID, "%s: null fixed", who);
    for (int i = 0; i < n_fixed; i++) {
        VELO_TRY(check_frame(fixed[i], who));
        if (i > 0 && fixed[i] <= fixed[i - 1]) return fail(VELO_ERR_INVALID, "%s: fixed frames must be ascending and distinct (%d after %d)", who, fixed[i], fixed[i - 1]);
    }
    if (params) {
        if (!(params->cg_tolerance > 0.0 && params->cg_tolerance < 1.0)) return fail(VELO_ERR_INVALID, "%s: cg_tolerance must lie in (0, 1)", who);
        if (params->cg_max_iterations < 1) return fail(VELO_ERR_INVALID, "%s: cg_max_iterations %d; at least 1", who, params->cg_max_iterations);
        if (params->reserved[0] != VELO_GRAPH_SOLVER_CG && params->reserved[0] != VELO_GRAPH_SOLVER_ENVELOPE)
            return fail(VELO_ERR_INVALID, "%s: linear solver %d (reserved[0]); 0 (CG) or 1 (envelope)", who, params->reserved[0]);
        if (params->reserved[1] < 0) return fail(VELO_ERR_INVALID, "%s: negative work cap %d (reserved[1])", who, params->reserved[1]);
    }
    VELO_TRY(graph_need_store(c, who));
    const GraphStore& S = *c->graph;
    for (int i = 0; i < n_fixed; i++)
        if (!graph_has_pose(S, fixed[i])) return fail(VELO_ERR_STATE, "%s: fixed frame %d has no pose: velo_graph_set_pose", who, fixed[i]);
    for (size_t e = 0; e < S.n_edges; e++) {
        const int32_t ends[2] = {S.h_from[e], S.h_to[e]};
        for (int k = 0; k < 2; k++)
            if (!graph_has_pose(S, ends[k])) return fail(VELO_ERR_STATE, "%s: edge %zu ends at frame %d, which has no pose", who, e, ends[k]);
    }
    return VELO_OK;
}

// the linearisation of buffer `which`: a store that has never seen a weighted edge runs the scalar kernel
void graph_linearize(velo_ctx* c, const GraphArgs& A, const GraphWeights& W, int which) {
    const dim3 grid((unsigned)std::max(1, cdiv(A.E, kGrThreads)));
    if (W.winfo) hipLaunchKernelGGL(graph_linearize_weighted_kernel, grid, dim3(kGrThreads), 0, c->stream, A, W, which);
    else hipLaunchKernelGGL(graph_linearize_kernel, grid, dim3(kGrThreads), 0, c->stream, A, which);
}

// the free nodes, their incidence lists (ints only), the poses to both buffers; then the system at the stored state: linearise,
// assemble, reduce
int graph_begin(velo_ctx* c, const int32_t* fixed, int32_t n_fixed, const velo_graph_params& params, GraphCall* call) {
    GraphStore& S = *c->graph;
    HIP_TRY(hipSetDevice(c->device));
    const size_t F = S.frame_cap, E = S.n_edges;
    std::vector<int32_t> slot(F, -1);
    std::vector<int32_t>& nodes = call->free_nodes;
    nodes.clear();
    for (size_t f = 0, k = 0; f < F; f++) {
        while (k < (size_t)n_fixed && (size_t)fixed[k] < f) k++;
        if (S.pose_set[f] && !(k < (size_t)n_fixed && (size_t)fixed[k] == f)) { slot[f] = (int32_t)nodes.size(); nodes.push_back((int32_t)f); }
    }
    const size_t n = nodes.size();
    std::vector<int32_t> start(n + 1, 0), inc, other;
    for (size_t e = 0; e < E; e++) {
        if (slot[(size_t)S.h_from[e]] >= 0) start[(size_t)slot[(size_t)S.h_from[e]] + 1]++;
        if (slot[(size_t)S.h_to[e]] >= 0) start[(size_t)slot[(size_t)S.h_to[e]] + 1]++;
    }
    for (size_t i = 0; i < n; i++) start[i + 1] += start[i];
    inc.resize((size_t)start[n]);
    other.resize(inc.size());
    {
        std::vector<int32_t> fill(start.begin(), start.end() - 1);
        for (size_t e = 0; e < E; e++) {                               // ascending edge number within every node: the fixed order
            const int32_t sf = slot[(size_t)S.h_from[e]], st = slot[(size_t)S.h_to[e]];
            if (sf >= 0) { const size_t k = (size_t)fill[(size_t)sf]++; inc[k] = (int32_t)(2 * e); other[k] = st; }
            if (st >= 0) { const size_t k = (size_t)fill[(size_t)st]++; inc[k] = (int32_t)(2 * e + 1); other[k] = sf; }
        }
    }
    // the envelope solver's order of the free nodes (velo_graph_order on the edges between two of them), refused here -- before anything is
    // sent -- when its work exceeds the cap; ints: perm, pos, first, rowptr, last
    std::vector<int32_t>& env_ints = call->env_ints;
    env_ints.clear();
    if (call->envelope && n) {
        std::vector<int32_t> ea, eb, perm(n), first(n);
        for (size_t e = 0; e < E; e++) {
            const int32_t sf = slot[(size_t)S.h_from[e]], st = slot[(size_t)S.h_to[e]];
            if (sf >= 0 && st >= 0) { ea.push_back(sf); eb.push_back(st); }
        }
        graph_order((int32_t)n, (int32_t)ea.size(), ea.data(), eb.data(), perm.data(), first.data(), call->env_stats);
        VELO_TRY(graph_env_refusal(call->who, call->env_stats, call->max_work, n, "raise reserved[1] or use the CG solver"));
        graph_env_ints(n, perm.data(), first.data(), &env_ints);
    }
    const int nb = std::max(1, cdiv((int)n, kGrThreads));
    call->n_free = (int)n; call->E = (int)E;
    VELO_TRY(S.node.reserve(n + 1));
    VELO_TRY(S.inc_start.reserve(n + 1));
    VELO_TRY(S.inc.reserve(2 * inc.size() + 1));
    VELO_TRY(S.x.reserve(2 * F * 6 + 1));
    VELO_TRY(S.blk.reserve(2 * E * kGrBlk + 1));
    if (S.weighted) VELO_TRY(S.estat.reserve(2 * E * 2 + 1));
    VELO_TRY(S.nd.reserve(2 * n * kGrNode + 1));
    VELO_TRY(S.vec.reserve(n * kGraphVec + 1));
    VELO_TRY(S.part.reserve(4 * (size_t)nb));
    VELO_TRY(S.nterm.reserve(2 * n + 1));
    VELO_TRY(S.rec.reserve(1));
    VELO_TRY(S.h_out.reserve(sizeof(GraphRecord) + sizeof(double) * std::max(F * 6, n * kGrNode) + 64));
    const size_t n_ints = n + (n + 1) + 2 * inc.size();
    if (!env_ints.empty()) {
        VELO_TRY(S.env_idx.reserve(env_ints.size()));
        VELO_TRY(S.env.reserve((size_t)call->env_stats[1] * 36));
    }
    VELO_TRY(S.h_st.reserve(sizeof(int32_t) * (n_ints + env_ints.size() + 1)));
    int32_t* st = (int32_t*)S.h_st.p;
    if (!env_ints.empty()) {
        std::memcpy(st + n_ints, env_ints.data(), sizeof(int32_t) * env_ints.size());
        HIP_TRY(hipMemcpyAsync(S.env_idx.p, st + n_ints, sizeof(int32_t) * env_ints.size(), hipMemcpyHostToDevice, c->stream));
    }
    if (n) std::memcpy(st, nodes.data(), sizeof(int32_t) * n);
    std::memcpy(st + n, start.data(), sizeof(int32_t) * (n + 1));
    if (!inc.empty()) {                                                // inc, then inc_other behind it, in one copy
        std::memcpy(st + n + n + 1, inc.data(), sizeof(int32_t) * inc.size());
        std::memcpy(st + n + n + 1 + inc.size(), other.data(), sizeof(int32_t) * inc.size());
    }
    if (n) HIP_TRY(hipMemcpyAsync(S.node.p, st, sizeof(int32_t) * n, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(S.inc_start.p, st + n, sizeof(int32_t) * (n + 1), hipMemcpyHostToDevice, c->stream));
    if (!inc.empty()) HIP_TRY(hipMemcpyAsync(S.inc.p, st + n + n + 1, sizeof(int32_t) * 2 * inc.size(), hipMemcpyHostToDevice, c->stream));
    if (F) {
        HIP_TRY(hipMemcpyAsync(S.x.p, S.h_x.p, sizeof(double) * F * 6, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(S.x.p + F * 6, S.h_x.p, sizeof(double) * F * 6, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(hipMemsetAsync(S.rec.p, 0, sizeof(GraphRecord), c->stream));
    if (n) HIP_TRY(hipMemsetAsync(S.nterm.p, 0, sizeof(double) * 2 * n, c->stream));
    GraphArgs& A = call->A;
    std::memset(&A, 0, sizeof(A));
    A.from = S.from.p; A.to = S.to.p; A.z = S.z.p; A.info = S.info.p;
    A.x = S.x.p; A.x_stride = F * 6;
    A.node = S.node.p; A.inc_start = S.inc_start.p; A.inc = S.inc.p; A.inc_other = S.inc.p + inc.size();
    A.blk = S.blk.p; A.nd = S.nd.p;
    double* v = S.vec.p;
    A.scale = v; v += n * 6;
    A.diag = v; v += n * 6;
    A.chol = v; v += n * 21;
    A.y = v; v += n * 6;
    A.r = v; v += n * 6;
    A.zv = v; v += n * 6;
    A.q = v; v += n * 6;
    A.p = v;
    A.part_rho0 = S.part.p; A.part_rho = S.part.p + nb; A.part_sigma = S.part.p + 3 * (size_t)nb;
    A.nterm = S.nterm.p; A.rec = S.rec.p;
    A.E = (int)E; A.n_free = (int)n; A.nb = nb;
    if (!env_ints.empty()) graph_env_bind(&A, S.env_idx.p, n, S.env.p);
    if (S.weighted) { call->W.winfo = S.winfo.p; call->W.loss = S.wloss.p; call->W.estat = S.estat.p; }
    A.cg_tol2 = params.cg_tolerance * params.cg_tolerance;
    A.lm = lm_params(c->P);
    if (E) graph_linearize(c, A, call->W, 0);
    if (n) hipLaunchKernelGGL(graph_assemble_kernel, dim3((unsigned)nb), dim3(kGrThreads), 0, c->stream, A, 0, 0);
    hipLaunchKernelGGL(graph_reduce_kernel, dim3(kGrRed), dim3(256), 0, c->stream, A, 0);
    HIP_TRY(hipGetLastError());
    return VELO_OK;
}

int graph_read_record(velo_ctx* c, GraphStore& S, GraphRecord** rec) {
    HIP_TRY(hipMemcpyAsync(S.h_out.p, S.rec.p, sizeof(GraphRecord), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *rec = (GraphRecord*)S.h_out.p;
    return VELO_OK;
}

int graph_put_poses(velo_ctx* c, int32_t first, int32_t n, const double* poses, const char* who) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    if (n < 0) return fail(VELO_ERR_INVALID, "%s: negative count", who);
    if (first < 0 || (int64_t)first + n > kLmMaxFrame) return fail(VELO_ERR_INVALID, "%s: frames %d .. %lld; 0..%d", who, first, (long long)first + n - 1, kLmMaxFrame - 1);
    if (n > 0 && !poses) return fail(VELO_ERR_INVALID, "%s: null poses", who);
    for (size_t k = 0; k < 6 * (size_t)n; k++) if (!std::isfinite(poses[k])) return fail(VELO_ERR_INVALID, "%s: pose %zu, entry %zu is not finite", who, k / 6, k % 6);
    VELO_TRY(graph_need_store(c, who));
    if (n == 0) return VELO_OK;
    GraphStore& S = *c->graph;
    HIP_TRY(hipSetDevice(c->device));
    const size_t last = (size_t)first + (size_t)n;
    for (size_t f = (size_t)first; f < last && S.ret.state != 0; f++) {   // a retained factorisation: a frame that has a pose moves, or a new one
        const bool posed = graph_has_pose(S, (int64_t)f);              // below a retained free frame shifts the free indices: dropped
        if (posed || (!S.ret.free_nodes.empty() && (int64_t)f < S.ret.free_nodes.back())) graph_ret_drop(S);
        else graph_ret_behind(S);
    }
    if (last > S.frame_cap) {                                         // the table grows geometrically: a new pinned mirror, filled from the old one
        const size_t cap = std::max<size_t>({last, 2 * S.frame_cap, 256});
        PinBuf<double> nh;
        VELO_TRY(nh.reserve(sizeof(double) * cap * 6));
        std::memset(nh.p, 0, sizeof(double) * cap * 6);
        if (S.h_x.p) std::memcpy(nh.p, S.h_x.p, sizeof(double) * S.frame_cap * 6);      // (no copy out of it is in flight: every call that sends it synchronises)
        S.h_x = std::move(nh);
        S.frame_cap = cap;
        S.pose_set.resize(cap, 0);
    }
    std::memcpy(S.h_x.p + (size_t)first * 6, poses, sizeof(double) * 6 * (size_t)n);
    for (size_t f = (size_t)first; f < last; f++) if (!S.pose_set[f]) { S.pose_set[f] = 1; S.n_nodes++; }
    return VELO_OK;
}

// what every entry that appends edges refuses of edge e's ends and measurement
int graph_check_edge(int e, const int32_t* from, const int32_t* to, const double* z) {
    if (from[e] < 0 || from[e] >= kLmMaxFrame || to[e] < 0 || to[e] >= kLmMaxFrame) return fail(VELO_ERR_INVALID, "edge %d: frames %d -> %d; 0..%d", e, from[e], to[e], kLmMaxFrame - 1);
    if (from[e] == to[e]) return fail(VELO_ERR_INVALID, "edge %d: from == to (%d)", e, from[e]);
    for (int k = 0; k < 6; k++) if (!std::isfinite(z[6 * (size_t)e + k])) return fail(VELO_ERR_INVALID, "edge %d: z[%d] is not finite", e, k);
    return VELO_OK;
}

// W = L L^T in double from W's upper triangle (row by row); L: the lower triangle, row-major packed.  False for a pivot that is not
// positive and finite.
bool graph_host_chol6(const double* upper21, double* L21) {
    double M[36];
    for (int i = 0, o = 0; i < 6; i++)
        for (int j = i; j < 6; j++, o++) M[i * 6 + j] = M[j * 6 + i] = upper21[o];
    for (int j = 0; j < 6; j++) {
        double dj = M[j * 6 + j];
        for (int k = 0; k < j; k++) dj -= M[j * 6 + k] * M[j * 6 + k];
        if (!(dj > 0.0) || !std::isfinite(dj)) return false;
        const double l = std::sqrt(dj);
        M[j * 6 + j] = l;
        for (int i = j + 1; i < 6; i++) {
            double acc = M[i * 6 + j];
            for (int k = 0; k < j; k++) acc -= M[i * 6 + k] * M[j * 6 + k];
            M[i * 6 + j] = acc / l;
            if (!std::isfinite(M[i * 6 + j])) return false;
        }
    }
    for (int i = 0, o = 0; i < 6; i++)
        for (int j = 0; j <= i; j++, o++) L21[o] = M[i * 6 + j];
    return true;
}

// appends n checked edges: scalar ones (info) or weighted ones (L: 21 doubles per edge, loss: one).  The first weighted edge turns the
// store into a weighted one: its columns are allocated and the scalar edges it holds are restated there.
int graph_append(velo_ctx* c, int32_t n, const int32_t* from, const int32_t* to, const double* z, const double* info, const double* L, const double* loss) {
    GraphStore& S = *c->graph;
    if (S.n_edges + (size_t)n > (size_t)(1 << 30)) return fail(VELO_ERR_INVALID, "more than 2^30 edges");
    HIP_TRY(hipSetDevice(c->device));
    if (L && !S.weighted) graph_ret_drop(S);                           // the promotion restates every edge
    else graph_ret_behind(S);
    if (L && !S.weighted) {
        VELO_TRY(S.winfo.reserve(S.edge_cap * 21));
        VELO_TRY(S.wloss.reserve(S.edge_cap));
        if (S.n_edges) {
            hipLaunchKernelGGL(graph_promote_kernel, dim3((unsigned)cdiv((int)S.n_edges, kGrThreads)), dim3(kGrThreads), 0, c->stream, S.info.p, S.winfo.p, S.wloss.p, 0, (int)S.n_edges);
            HIP_TRY(hipGetLastError());
        }
        S.weighted = true;
    }
    const size_t need = S.n_edges + (size_t)n;
    if (need > S.edge_cap) {                                           // grow by doubling; what is there is kept
        size_t cap = S.edge_cap;
        while (cap < need) cap *= 2;
        VELO_TRY(lm_regrow(c, &S.from, S.n_edges, cap, 0));
        VELO_TRY(lm_regrow(c, &S.to, S.n_edges, cap, 0));
        VELO_TRY(lm_regrow(c, &S.z, S.n_edges * 6, cap * 6, 0));
        VELO_TRY(lm_regrow(c, &S.info, S.n_edges, cap, 0));
        if (S.weighted) {
            VELO_TRY(lm_regrow(c, &S.winfo, S.n_edges * 21, cap * 21, 0));
            VELO_TRY(lm_regrow(c, &S.wloss, S.n_edges, cap, 0));
        }
        S.edge_cap = cap;
        S.edge_reallocs++;
    }
    const size_t nz = (size_t)n, per = info ? 1 : 22, bytes = nz * (2 * sizeof(int32_t) + (6 + per) * sizeof(double));
    VELO_TRY(S.in_ev.wait_or_create());
    VELO_TRY(S.h_in.reserve(bytes));
    double* hz = (double*)S.h_in.p;
    double* hi = hz + 6 * nz;                                          // info [n], or L [n][21] and the loss scales [n] behind it
    int32_t* hf = (int32_t*)(hi + per * nz);
    int32_t* ht = hf + nz;
    std::memcpy(hz, z, sizeof(double) * 6 * nz);
    if (info) std::memcpy(hi, info, sizeof(double) * nz);
    else { std::memcpy(hi, L, sizeof(double) * 21 * nz); std::memcpy(hi + 21 * nz, loss, sizeof(double) * nz); }
    std::memcpy(hf, from, sizeof(int32_t) * nz);
    std::memcpy(ht, to, sizeof(int32_t) * nz);
    HIP_TRY(hipMemcpyAsync(S.z.p + 6 * S.n_edges, hz, sizeof(double) * 6 * nz, hipMemcpyHostToDevice, c->stream));
    if (info) HIP_TRY(hipMemcpyAsync(S.info.p + S.n_edges, hi, sizeof(double) * nz, hipMemcpyHostToDevice, c->stream));
    else {
        HIP_TRY(hipMemcpyAsync(S.winfo.p + 21 * S.n_edges, hi, sizeof(double) * 21 * nz, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipMemcpyAsync(S.wloss.p + S.n_edges, hi + 21 * nz, sizeof(double) * nz, hipMemcpyHostToDevice, c->stream));
    }
    HIP_TRY(hipMemcpyAsync(S.from.p + S.n_edges, hf, sizeof(int32_t) * nz, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(S.to.p + S.n_edges, ht, sizeof(int32_t) * nz, hipMemcpyHostToDevice, c->stream));
    if (info && S.weighted) {                                          // a scalar edge in a weighted store
        hipLaunchKernelGGL(graph_promote_kernel, dim3((unsigned)cdiv(n, kGrThreads)), dim3(kGrThreads), 0, c->stream, S.info.p, S.winfo.p, S.wloss.p, (int)S.n_edges, n);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipEventRecord(S.in_ev, c->stream));
    S.h_from.insert(S.h_from.end(), from, from + n);
    S.h_to.insert(S.h_to.end(), to, to + n);
    S.n_edges = need;
    return VELO_OK;
}

// ---- what velo_graph_covariance, velo_graph_edge_gate and velo_graph_loop_candidates share behind graph_begin -----------------------------
constexpr size_t kGraphRecDoubles = sizeof(GraphRecord) / sizeof(double);     // a call's record heads S.cov_out, its results follow
static_assert(sizeof(GraphRecord) % sizeof(double) == 0, "a call's results follow its record");

// H~ of the stored state (all of A's rows) and the factor of its leading `rows` rows, A's record cleared before
int graph_cov_factor(velo_ctx* c, const GraphArgs& A, int rows) {
    GraphArgs B = A;
    B.n_free = rows;
    HIP_TRY(hipMemsetAsync(A.rec, 0, sizeof(GraphRecord), c->stream));
    hipLaunchKernelGGL(graph_env_fill_undamped_kernel, dim3((unsigned)A.n_free), dim3(64), 0, c->stream, A);
    hipLaunchKernelGGL(graph_env_factor_kernel, dim3(1), dim3(kGrEnvFactorThreads), 0, c->stream, B);
    HIP_TRY(hipGetLastError());
    return VELO_OK;
}

// The refusal of a call whose factor met a pivot that is not positive and finite.  Which pivot: the factor of the leading k rows fails exactly
// when k exceeds the first bad pivot's position, so bisect on k.  A refusal's path only: each probe fills and factors again.
int graph_cov_refuse(velo_ctx* c, const std::vector<int32_t>& free_nodes, const int32_t* perm, const GraphArgs& A, const char* who) {
    GraphStore& S = *c->graph;
    int lo = 0, hi = (int)free_nodes.size();
    while (hi - lo > 1) {
        const int mid = lo + (hi - lo) / 2;
        VELO_TRY(graph_cov_factor(c, A, mid));
        HIP_TRY(hipMemcpyAsync(S.h_out.p, A.rec, sizeof(GraphRecord), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (((const GraphRecord*)S.h_out.p)->bad != 0) hi = mid; else lo = mid;
    }
    return fail(VELO_ERR_INVALID, "%s: J^T J is not positive definite: the factorisation's pivot at frame %d (position %d of the order) is not positive and finite; "
                "every free node needs edges that determine it", who, free_nodes[(size_t)perm[(size_t)hi - 1]], hi - 1);
}

// the cap on a call's column work vectors; what: what a column is solved for, in the refusal's words
int graph_column_cap(velo_ctx* c, const char* who, const char* what, size_t n_cols, size_t n) {
    if (n_cols * n * 36 <= (size_t)VELO_GRAPH_MAX_COLUMN_DOUBLES) return VELO_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));                          // (graph_begin's copies out of the staging are done before the next call fills it)
    return fail(VELO_ERR_INVALID, "%s: %zu %s need %zu doubles of work vectors (%zu free nodes x 36 each), over the cap of %lld; ask in smaller batches",
                who, n_cols, what, n_cols * n * 36, n, (long long)VELO_GRAPH_MAX_COLUMN_DOUBLES);
}

// ---- the retained factorisation (velo_graph_retain) ----------------------------------------------------------------------------------------
// the edges between two free nodes in free indices, in the store's order, and how many of them lie among the store's first `seen` edges
void graph_free_edges(const GraphStore& S, const std::vector<int32_t>& free_nodes, size_t seen, std::vector<int32_t>* ea, std::vector<int32_t>* eb, size_t* n_seen,
                      std::vector<int32_t>* slot_out) {
    std::vector<int32_t>& slot = *slot_out;
    slot.assign(S.frame_cap, -1);
    for (size_t i = 0; i < free_nodes.size(); i++) slot[(size_t)free_nodes[i]] = (int32_t)i;
    ea->clear(); eb->clear();
    *n_seen = 0;
    for (size_t e = 0; e < S.n_edges; e++) {
        const int32_t sf = slot[(size_t)S.h_from[e]], st = slot[(size_t)S.h_to[e]];
        if (sf >= 0 && st >= 0) { ea->push_back(sf); eb->push_back(st); if (e < seen) ++*n_seen; }
    }
}

// the kernels' arguments over the retained buffers: what the selected inverse, the columns and the pairs' kernels read
GraphArgs graph_ret_args(const GraphRetained& R) {
    GraphArgs A;
    std::memset(&A, 0, sizeof(A));
    const size_t n = R.free_nodes.size();
    A.x = R.x.p; A.x_stride = R.frames * 6;
    A.scale = R.scale.p; A.n_free = (int)n;
    graph_env_bind(&A, R.idx.p, n, R.env.p);
    return A;
}

// Builds (p_rule < 0: every row, in the order `ints`) or extends (rows >= p) the retained factor from the system graph_begin has just formed
// in the store's work buffers.  *bad: a pivot was not positive and finite; the rows >= p are then not valid.  Nothing of R's host state moves.
int graph_ret_factor(velo_ctx* c, GraphRetained& R, const GraphCall& call, const std::vector<int32_t>& ints, int64_t blocks, int p, size_t keep_blocks, bool* bad, GraphArgs* out) {
    GraphStore& S = *c->graph;
    const size_t n = (size_t)call.n_free, F = S.frame_cap;
    VELO_TRY(R.idx.reserve(ints.size() + 1));
    VELO_TRY(R.scale.reserve(n * 6 + 1));
    VELO_TRY(R.x.reserve(F * 6 + 1));
    if ((size_t)blocks * 36 + 1 > R.env.cap) {                         // (DevBuf::reserve frees on growth: the rows that keep their factor are carried over)
        if (keep_blocks) VELO_TRY(lm_regrow(c, &R.env, keep_blocks * 36, (size_t)blocks * 36 + 1, 0));
        else VELO_TRY(R.env.reserve((size_t)blocks * 36 + 1));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));                          // (the last copy out of h_idx is done)
    VELO_TRY(R.h_idx.reserve(sizeof(int32_t) * (ints.size() + 1)));
    std::memcpy(R.h_idx.p, ints.data(), sizeof(int32_t) * ints.size());
    // INVARIANT: idx, scale and x on the device are the ATTEMPTED generation's from here on, while R.ints and R.free_nodes stay the old one's
    // until graph_ret_commit.  A failed extension leaves them apart.  That is safe because a state that is behind is never served
    // (graph_query_open) and every build or extension passes here, uploading all three again before anything reads them.
    HIP_TRY(hipMemcpyAsync(R.idx.p, R.h_idx.p, sizeof(int32_t) * ints.size(), hipMemcpyHostToDevice, c->stream));
    if (n) HIP_TRY(hipMemcpyAsync(R.scale.p, call.A.scale, sizeof(double) * n * 6, hipMemcpyDeviceToDevice, c->stream));
    if (F) HIP_TRY(hipMemcpyAsync(R.x.p, call.A.x, sizeof(double) * F * 6, hipMemcpyDeviceToDevice, c->stream));
    GraphArgs A = call.A;                                              // the system (blk, nd, inc) is the store's, the skyline and its ints are R's
    A.scale = R.scale.p;
    graph_env_bind(&A, R.idx.p, n, R.env.p);
    *out = A;
    *bad = false;
    if (n == 0 || p >= (int)n) return VELO_OK;
    if (p <= 0) VELO_TRY(graph_cov_factor(c, A, (int)n));
    else {
        int k0 = p;
        for (size_t i = (size_t)p; i < n; i++) k0 = std::min(k0, ints[2 * n + i]);
        HIP_TRY(hipMemsetAsync(A.rec, 0, sizeof(GraphRecord), c->stream));
        hipLaunchKernelGGL(graph_env_fill_undamped_rows_kernel, dim3((unsigned)(n - (size_t)p)), dim3(64), 0, c->stream, A, p);
        hipLaunchKernelGGL(graph_env_factor_rows_kernel, dim3(1), dim3(kGrEnvFactorThreads), 0, c->stream, A, p, k0);
        HIP_TRY(hipGetLastError());
    }
    HIP_TRY(hipMemcpyAsync(S.h_out.p, A.rec, sizeof(GraphRecord), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    *bad = ((const GraphRecord*)S.h_out.p)->bad != 0;
    return VELO_OK;
}

void graph_ret_commit(GraphStore& S, GraphRetained& R, const GraphCall& call, std::vector<int32_t>& ints, const int64_t* stats) {
    R.free_nodes = call.free_nodes;
    R.ints.swap(ints);
    for (int k = 0; k < 4; k++) R.stats[k] = stats[k];
    R.edges_seen = S.n_edges; R.frames = S.frame_cap;
    R.valid_rows = call.n_free;
    R.z_valid = false; R.col_pos = -1;
    R.state = 1;
}

// a state that is behind: the order of velo_graph_order_extend, the system again, the rows from the first dirty one on.  *ok false: the
// extension failed (the cap, a pivot) and the state stays behind at its last generation; the caller answers by the un-retained path.
int graph_ret_extend(velo_ctx* c, bool* ok) {
    GraphStore& S = *c->graph;
    GraphRetained& R = S.ret;
    *ok = false;
    GraphCall call;
    call.who = "velo_graph_retain";
    VELO_TRY(graph_begin(c, R.fixed.data(), (int32_t)R.fixed.size(), graph_params(nullptr), &call));
    const size_t n_old = R.free_nodes.size(), n = (size_t)call.n_free;
    if (n < n_old || !std::equal(R.free_nodes.begin(), R.free_nodes.end(), call.free_nodes.begin())) {      // (the hooks keep this from happening)
        graph_ret_drop(S);
        HIP_TRY(hipStreamSynchronize(c->stream));
        return VELO_OK;
    }
    std::vector<int32_t> ea, eb, slot, perm(n), first(n), ints;
    size_t m_old = 0;
    graph_free_edges(S, call.free_nodes, R.edges_seen, &ea, &eb, &m_old, &slot);
    int64_t st[8];
    if (!graph_order_extend((int32_t)n_old, R.ints.data(), (int32_t)n, (int32_t)ea.size(), ea.data(), eb.data(), (int32_t)m_old, R.max_work, perm.data(), first.data(), st)) {
        graph_ret_drop(S);
        HIP_TRY(hipStreamSynchronize(c->stream));
        return VELO_OK;
    }
    if (st[2] > R.max_work || st[1] > (int64_t)1 << 30) { HIP_TRY(hipStreamSynchronize(c->stream)); return VELO_OK; }
    graph_env_ints(n, perm.data(), first.data(), &ints);
    int p = (int)st[4];
    for (size_t e = R.edges_seen; e < S.n_edges; e++) {                // a new edge to a constant changes its free end's diagonal block
        const int32_t sf = slot[(size_t)S.h_from[e]], sb = slot[(size_t)S.h_to[e]];
        if ((sf >= 0) != (sb >= 0)) p = std::min(p, ints[n + (size_t)(sf >= 0 ? sf : sb)]);
    }
    const bool rebuilt = st[5] != 0;
    if (!rebuilt) p = std::min(p, R.valid_rows);
    bool bad = false;
    GraphArgs A;
    VELO_TRY(graph_ret_factor(c, R, call, ints, st[1], p, !rebuilt && p > 0 ? (size_t)ints[3 * n + (size_t)p] : 0, &bad, &A));
    if (bad) { R.valid_rows = rebuilt ? 0 : std::min(R.valid_rows, p); return VELO_OK; }
    graph_ret_commit(S, R, call, ints, st);
    R.counters[1]++;
    if (rebuilt) R.counters[2]++;
    R.last_p = p; R.last_rows = (int64_t)n - p;
    *ok = true;
    return VELO_OK;
}

// Room for nc full columns in R.col, the kept one staying in slot 0.  cols: the positions the call needs; on return cols[0] is the kept
// column when the call needs it (*first_new = 1: solve the slots from 1 on), otherwise the call's last one (*first_new = 0).  remap:
// the slot of each entry of the caller's numbering, the identity on entry.
int graph_ret_columns(velo_ctx* c, GraphRetained& R, std::vector<int32_t>& cols, std::vector<int32_t>* remap, int* first_new) {
    const size_t nc = cols.size(), n = R.free_nodes.size();
    *first_new = 0;
    if (nc == 0) return VELO_OK;
    size_t at = nc - 1;
    for (size_t k = 0; k < nc; k++) if (R.col_pos >= 0 && cols[k] == R.col_pos) { at = k; *first_new = 1; }
    std::swap(cols[0], cols[at]);
    (*remap)[0] = (int32_t)at; (*remap)[at] = 0;
    if (nc * n * 36 + 1 > R.col.cap) {
        if (*first_new) VELO_TRY(lm_regrow(c, &R.col, n * 36, nc * n * 36 + 1, 0));
        else { R.col_pos = -1; VELO_TRY(R.col.reserve(nc * n * 36 + 1)); }
    }
    return VELO_OK;
}

// ---- the factor a query reads: velo_graph_covariance, velo_graph_edge_gate and velo_graph_loop_candidates between their own packing and kernel ----
// What a query needs of the factorisation and nothing about where it lives.  Two producers (graph_query_open): the retained state, whose
// ints and free nodes it refers to, or a build for this call in the store's buffers (`built` holds its host side).  As declared it is the
// factor of no system (n = 0), which is what velo_graph_loop_candidates without sigma asks with.
struct GraphFactor {
    GraphArgs A;                                         // over the buffers of either home; rec: the call's record (graph_query_reserve)
    GraphRetained* kept = nullptr;                       // the retained state, or null: built for this call
    GraphCall built;
    size_t n = 0;                                        // free nodes
    const std::vector<int32_t>* free_nodes = &built.free_nodes;
    const int32_t *perm = nullptr, *pos = nullptr, *first = nullptr;      // of the order: position -> free index, its inverse, a row's first column
    const int64_t* stats = built.env_stats;              // widest row, blocks, work, components
    // from graph_query_reserve on
    double *zenv = nullptr, *work = nullptr;             // the selected inverse's skyline; the base of the columns' work vectors
    size_t n_res = 0, n_full = 0;                        // doubles of the record and the results; full columns the call needs
    int first_new = 0, col_pos = -1;                     // the slot from which they are solved (those before are held); the position of slot 0's
    bool run_selinv = false;                             // (retained) the generation's selected inverse is not there yet
    GraphFactor() { std::memset(&A, 0, sizeof(A)); }
    GraphFactor(const GraphFactor&) = delete;            // (it points into itself)
    int free_index(int32_t frame) const {                // -1: a constant
        const auto it = std::lower_bound(free_nodes->begin(), free_nodes->end(), frame);
        return it != free_nodes->end() && *it == frame ? (int)(it - free_nodes->begin()) : -1;
    }
    // the block of two free nodes lies outside the envelope: Z does not hold it, a column solve does
    bool outside(int32_t ia, int32_t ib) const { return first[(size_t)std::max(pos[(size_t)ia], pos[(size_t)ib])] > std::min(pos[(size_t)ia], pos[(size_t)ib]); }
};

// Open: the retained state where it is of this `fixed` set and no tighter cap is asked (a tighter one: the per-call path decides), extended
// first where it is behind -- a state that stays behind is never served; otherwise graph_begin's system and order for this call.
int graph_query_open(velo_ctx* c, const int32_t* fixed, int32_t n_fixed, const velo_graph_params* params, const char* who, GraphFactor* Q) {
    GraphRetained& R = c->graph->ret;
    const int64_t cap = graph_work_cap(params);
    bool serve = R.state != 0 && R.fixed.size() == (size_t)n_fixed && std::equal(R.fixed.begin(), R.fixed.end(), fixed) && cap >= R.max_work;
    if (serve) {
        HIP_TRY(hipSetDevice(c->device));
        if (R.state == 2) VELO_TRY(graph_ret_extend(c, &serve));
    }
    const int32_t* ints = R.ints.data();
    if (serve) { Q->kept = &R; Q->A = graph_ret_args(R); Q->free_nodes = &R.free_nodes; Q->stats = R.stats; }
    else {
        Q->built.envelope = true; Q->built.who = who; Q->built.max_work = cap;
        VELO_TRY(graph_begin(c, fixed, n_fixed, graph_params(nullptr), &Q->built));
        Q->A = Q->built.A;
        ints = Q->built.env_ints.data();
    }
    Q->n = Q->free_nodes->size();
    Q->perm = ints; Q->pos = ints + Q->n; Q->first = ints + 2 * Q->n;
    return VELO_OK;
}

// Plan and reserve: the call's record with n_res - kGraphRecDoubles results behind it (one copy to the host), the selected inverse, the
// columns.  cols: the positions of the full columns the call needs -- the retained state's own, the kept one staying in slot 0 (remap: the
// slot of each entry of the caller's numbering) -- or null: n_pair pair columns, which are the store's on either path.
int graph_query_reserve(velo_ctx* c, GraphFactor* Q, const char* who, const char* what, size_t n_res, size_t n_pair, std::vector<int32_t>* cols, std::vector<int32_t>* remap) {
    GraphStore& S = *c->graph;
    const size_t n = Q->n, nc = cols ? cols->size() : n_pair;
    VELO_TRY(graph_column_cap(c, who, what, nc, n));
    if (cols) { remap->resize(nc); for (size_t k = 0; k < nc; k++) (*remap)[k] = (int32_t)k; }
    if (cols && Q->kept) VELO_TRY(graph_ret_columns(c, *Q->kept, *cols, remap, &Q->first_new));
    else if (n) VELO_TRY(S.cov_work.reserve(nc * n * 36 + 1));
    Q->work = cols && Q->kept ? Q->kept->col.p : S.cov_work.p;
    if (cols && nc) { Q->n_full = nc; Q->col_pos = (*cols)[0]; }
    if (Q->kept) {
        Q->run_selinv = !Q->kept->z_valid && n != 0;
        if (Q->run_selinv) VELO_TRY(Q->kept->zenv.reserve((size_t)Q->stats[1] * 36 + 1));
    } else if (n) VELO_TRY(S.cov_z.reserve((size_t)Q->stats[1] * 36));
    Q->zenv = Q->kept ? Q->kept->zenv.p : S.cov_z.p;
    VELO_TRY(S.cov_out.reserve(n_res));
    VELO_TRY(S.h_out.reserve(sizeof(double) * n_res + 64));
    Q->A.rec = (GraphRecord*)S.cov_out.p;
    Q->n_res = n_res;
    return VELO_OK;
}

// Enqueue the factor side behind a cleared record: the selected inverse, once per generation, or the fill, the factor and the selected
// inverse; then the full columns the state does not hold (full; null: the caller solves its own kind).  pairs: velo_graph_covariance's,
// which its per-call selected inverse is launched with (the kernel reads zenv alone).
int graph_query_enqueue(velo_ctx* c, const GraphFactor& Q, const GraphCov* pairs, const GraphRel* full) {
    GraphCov Z;
    Z.zenv = Q.zenv; Z.work = nullptr; Z.pair = nullptr; Z.out = nullptr; Z.n_pairs = 0;
    HIP_TRY(hipMemsetAsync(Q.A.rec, 0, sizeof(GraphRecord), c->stream));
    if (Q.kept) {
        if (Q.run_selinv) hipLaunchKernelGGL(graph_env_selinv_kernel, dim3(1), dim3(kGrEnvSelinvThreads), 0, c->stream, Q.A, Z);
    } else if (Q.n) {
        VELO_TRY(graph_cov_factor(c, Q.A, (int)Q.n));
        hipLaunchKernelGGL(graph_env_selinv_kernel, dim3(1), dim3(kGrEnvSelinvThreads), 0, c->stream, Q.A, pairs ? *pairs : Z);
    }
    if (full && Q.n_full > (size_t)Q.first_new) {
        GraphRel R = *full;
        R.work += (size_t)Q.first_new * Q.n * 36; R.col_pos += Q.first_new;
        hipLaunchKernelGGL(graph_env_column_full_kernel, dim3((unsigned)(Q.n_full - (size_t)Q.first_new)), dim3(kGrEnvColumnThreads), 0, c->stream, Q.A, R);
    }
    return VELO_OK;
}

// Finish: the record and the results to S.h_out, the synchronisation, and what the call leaves behind -- on the retained state the selected
// inverse, the column in slot 0 and the counters; of a build for this call the refusal of a pivot that was not positive and finite.
int graph_query_finish(velo_ctx* c, const GraphFactor& Q, const char* who) {
    GraphStore& S = *c->graph;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(S.h_out.p, S.cov_out.p, sizeof(double) * Q.n_res, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (Q.kept) {
        GraphRetained& R = *Q.kept;
        R.z_valid = R.z_valid || Q.run_selinv; R.counters[3] += Q.run_selinv; R.counters[5]++;
        R.counters[4] += (int64_t)Q.n_full - Q.first_new;
        if (Q.n_full) R.col_pos = Q.col_pos;
    } else if (((const GraphRecord*)S.h_out.p)->bad != 0) return graph_cov_refuse(c, *Q.free_nodes, Q.perm, Q.A, who);
    return VELO_OK;
}

}  // namespace

extern "C" {   // (continued from the previous part)
int velo_default_graph_params(velo_graph_params* p) {
    if (!p) return fail(VELO_ERR_INVALID, "null params");
    std::memset(p, 0, sizeof(*p));
    // 1e-10: with it the inexact step takes the LM decisions of a direct solve on every graph tried, and its cost differs from the direct
    // solve's in the 11th digit; 2,000: four times what the longest solve of those graphs needed, a bound on the work of one LM iteration
    p->cg_tolerance = 1e-10;
    p->cg_max_iterations = 2000;
    return VELO_OK;
}

int velo_graph_reset(velo_ctx* c, int32_t edge_capacity) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    if (edge_capacity < 0) return fail(VELO_ERR_INVALID, "negative edge capacity");
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));           // nothing of the old store is in flight when it goes
    c->graph.reset();
    std::shared_ptr<GraphStore> S = std::make_shared<GraphStore>();
    const size_t want = edge_capacity > 0 ? (size_t)edge_capacity : kGraphDefaultEdges;
    VELO_TRY(S->from.reserve(want));
    VELO_TRY(S->to.reserve(want));
    VELO_TRY(S->z.reserve(want * 6));
    VELO_TRY(S->info.reserve(want));
    S->edge_cap = want;                                 // the buffers hold a little more; the arrays reallocate at what was asked for
    c->graph = S;
    return VELO_OK;
}

int velo_graph_set_pose(velo_ctx* c, int32_t frame, const double* pose6) { return graph_put_poses(c, frame, 1, pose6, "velo_graph_set_pose"); }

int velo_graph_set_poses(velo_ctx* c, int32_t first, int32_t n, const double* poses) { return graph_put_poses(c, first, n, poses, "velo_graph_set_poses"); }

int velo_graph_add_edges(velo_ctx* c, int32_t n, const int32_t* from, const int32_t* to, const double* z, const double* info) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    if (n < 0) return fail(VELO_ERR_INVALID, "negative edge count");
    if (n > 0 && (!from || !to || !z || !info)) return fail(VELO_ERR_INVALID, "null edge array");
    for (int e = 0; e < n; e++) {
        VELO_TRY(graph_check_edge(e, from, to, z));
        if (!(info[e] > 0.0 && std::isfinite(info[e]))) return fail(VELO_ERR_INVALID, "edge %d: info must be positive and finite", e);
    }
    VELO_TRY(graph_need_store(c, "velo_graph_add_edges"));
    if (n == 0) return VELO_OK;
    return graph_append(c, n, from, to, z, info, nullptr, nullptr);
}

int velo_graph_add_edges_weighted(velo_ctx* c, int32_t n, const int32_t* from, const int32_t* to, const double* z, const double* info21, const double* loss_scale) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    if (n < 0) return fail(VELO_ERR_INVALID, "negative edge count");
    if (n > 0 && (!from || !to || !z || !info21)) return fail(VELO_ERR_INVALID, "null edge array");
    std::vector<double> L(21 * (size_t)std::max(n, 0));
    for (int e = 0; e < n; e++) {
        VELO_TRY(graph_check_edge(e, from, to, z));
        const double* u = info21 + 21 * (size_t)e;
        for (int k = 0; k < 21; k++) if (!std::isfinite(u[k])) return fail(VELO_ERR_INVALID, "edge %d: info21[%d] is not finite", e, k);
        if (!graph_host_chol6(u, L.data() + 21 * (size_t)e)) return fail(VELO_ERR_INVALID, "edge %d: its information matrix is not positive definite (the Cholesky factorisation met a pivot that is not positive and finite)", e);
        if (loss_scale && !(loss_scale[e] >= 0.0 && std::isfinite(loss_scale[e]))) return fail(VELO_ERR_INVALID, "edge %d: loss_scale must be 0 (trivial) or positive and finite (Cauchy)", e);
    }
    VELO_TRY(graph_need_store(c, "velo_graph_add_edges_weighted"));
    if (n == 0) return VELO_OK;
    std::vector<double> zero;
    if (!loss_scale) { zero.assign((size_t)n, 0.0); loss_scale = zero.data(); }
    return graph_append(c, n, from, to, z, nullptr, L.data(), loss_scale);
}

int velo_graph_edge_stats(velo_ctx* c, int32_t first, int32_t n, double* chi2, double* weight) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    VELO_TRY(graph_need_store(c, "velo_graph_edge_stats"));
    GraphStore& S = *c->graph;
    if (first < 0 || n < 0 || (size_t)first + (size_t)n > S.n_edges) return fail(VELO_ERR_INVALID, "velo_graph_edge_stats: edges %d .. %lld; the store holds %zu", first, (long long)first + n - 1, S.n_edges);
    for (size_t e = (size_t)first; e < (size_t)first + (size_t)n; e++) {
        const int32_t ends[2] = {S.h_from[e], S.h_to[e]};
        for (int k = 0; k < 2; k++)
            if (!graph_has_pose(S, ends[k])) return fail(VELO_ERR_STATE, "velo_graph_edge_stats: edge %zu ends at frame %d, which has no pose", e, ends[k]);
    }
    if (n == 0) return VELO_OK;
    HIP_TRY(hipSetDevice(c->device));
    // the edges first .. first + n - 1 as a graph of their own: the stored poses to buffer 0, one linearisation there, which moves nothing
    const size_t F = S.frame_cap, E = S.n_edges, nz = (size_t)n;
    VELO_TRY(S.x.reserve(2 * F * 6 + 1));
    VELO_TRY(S.blk.reserve(2 * E * kGrBlk + 1));
    if (S.weighted) VELO_TRY(S.estat.reserve(2 * E * 2 + 1));
    VELO_TRY(S.h_out.reserve(sizeof(GraphRecord) + sizeof(double) * std::max(F * 6, 2 * nz) + 64));
    HIP_TRY(hipMemcpyAsync(S.x.p, S.h_x.p, sizeof(double) * F * 6, hipMemcpyHostToDevice, c->stream));
    GraphArgs A;
    std::memset(&A, 0, sizeof(A));
    A.from = S.from.p + first; A.to = S.to.p + first; A.z = S.z.p + 6 * (size_t)first; A.info = S.info.p + first;
    A.x = S.x.p; A.x_stride = F * 6; A.blk = S.blk.p; A.E = n;
    GraphWeights W = {nullptr, nullptr, nullptr};
    if (S.weighted) { W.winfo = S.winfo.p + 21 * (size_t)first; W.loss = S.wloss.p + first; W.estat = S.estat.p; }
    graph_linearize(c, A, W, 0);
    HIP_TRY(hipGetLastError());
    double* out = (double*)S.h_out.p;
    if (S.weighted) HIP_TRY(hipMemcpyAsync(out, S.estat.p, sizeof(double) * 2 * nz, hipMemcpyDeviceToHost, c->stream));
    else HIP_TRY(hipMemcpy2DAsync(out, sizeof(double), S.blk.p + kGrCost, sizeof(double) * kGrBlk, sizeof(double), nz, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (size_t k = 0; k < nz; k++) {                                  // a scalar store's cost term is info |r|^2 / 2 and its loss trivial
        if (chi2) chi2[k] = S.weighted ? out[2 * k] : 2.0 * out[k];
        if (weight) weight[k] = S.weighted ? out[2 * k + 1] : 1.0;
    }
    return VELO_OK;
}

int velo_graph_edge_information(const double z[6], const double JtJ36[36], double info21[21]) {
    if (!z || !JtJ36 || !info21) return fail(VELO_ERR_INVALID, "velo_graph_edge_information: null argument");
    for (int k = 0; k < 6; k++) if (!std::isfinite(z[k])) return fail(VELO_ERR_INVALID, "velo_graph_edge_information: z[%d] is not finite", k);
    for (int k = 0; k < 36; k++) if (!std::isfinite(JtJ36[k])) return fail(VELO_ERR_INVALID, "velo_graph_edge_information: JtJ36[%d] is not finite", k);
    // Bz^-1 = blockdiag(J_r^-1(w_z), Rz): Rz^T J_l(w) is the right Jacobian J_r(w), and J_r^-1 = I + K / 2 + (1 / t^2 - cot(t / 2) / (2 t)) K^2
    double T[16], M[36];
    VELO_TRY(velo_pose_vec_to_mat(z, T));
    const double x = z[0], y = z[1], w = z[2], t2 = x * x + y * y + w * w;
    double coef;
    if (t2 > 1e-6) {
        const double t = std::sqrt(t2);
        coef = 1.0 / t2 - std::cos(0.5 * t) / (2.0 * t * std::sin(0.5 * t));
    } else coef = 1.0 / 12.0 + t2 / 720.0;
    const double Ji[9] = {1.0 + coef * (x * x - t2), -0.5 * w + coef * x * y, 0.5 * y + coef * x * w,
                          0.5 * w + coef * x * y, 1.0 + coef * (y * y - t2), -0.5 * x + coef * y * w,
                          -0.5 * y + coef * x * w, 0.5 * x + coef * y * w, 1.0 + coef * (w * w - t2)};
    for (int k = 0; k < 36; k++) M[k] = 0.0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) { M[i * 6 + j] = Ji[i * 3 + j]; M[(3 + i) * 6 + 3 + j] = T[i * 4 + j]; }
    double HM[36];                                                     // ((H + H^T) / 2) M, then M^T of it
    for (int i = 0; i < 6; i++)
        for (int j = 0; j < 6; j++) {
            double acc = 0.0;
            for (int k = 0; k < 6; k++) acc += (0.5 * (JtJ36[i * 6 + k] + JtJ36[k * 6 + i])) * M[k * 6 + j];
            HM[i * 6 + j] = acc;
        }
    for (int i = 0, o = 0; i < 6; i++)
        for (int j = i; j < 6; j++, o++) {
            double a = 0.0, b = 0.0;                                   // (i, j) and (j, i), which differ by rounding only
            for (int k = 0; k < 6; k++) { a += M[k * 6 + i] * HM[k * 6 + j]; b += M[k * 6 + j] * HM[k * 6 + i]; }
            info21[o] = 0.5 * (a + b);
        }
    return VELO_OK;
}

int velo_graph_get_poses(velo_ctx* c, int32_t first, int32_t n, double* out) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    if (n < 0 || first < 0) return fail(VELO_ERR_INVALID, "velo_graph_get_poses: negative frame or count");
    if (n > 0 && !out) return fail(VELO_ERR_INVALID, "velo_graph_get_poses: null output");
    VELO_TRY(graph_need_store(c, "velo_graph_get_poses"));
    const GraphStore& S = *c->graph;
    for (int64_t f = first; f < (int64_t)first + n; f++)
        if (!graph_has_pose(S, f)) return fail(VELO_ERR_STATE, "velo_graph_get_poses: frame %lld has no pose", (long long)f);
    if (n > 0) std::memcpy(out, S.h_x.p + (size_t)first * 6, sizeof(double) * 6 * (size_t)n);
    return VELO_OK;
}

int velo_graph_info(velo_ctx* c, int32_t* info) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    if (!info) return fail(VELO_ERR_INVALID, "null info");
    VELO_TRY(graph_need_store(c, "velo_graph_info"));
    const GraphStore& S = *c->graph;
    info[0] = S.n_nodes; info[1] = (int32_t)S.n_edges; info[2] = (int32_t)S.edge_cap; info[3] = S.edge_reallocs;
    info[4] = (int32_t)S.frame_cap; info[5] = S.n_optimized; info[6] = S.env_widest; info[7] = S.env_blocks;
    return VELO_OK;
}

int velo_graph_order(int32_t n_nodes, int32_t n_edges, const int32_t* a, const int32_t* b, int32_t* perm, int32_t* first, int64_t* stats) {
    if (n_nodes < 0 || n_edges < 0) return fail(VELO_ERR_INVALID, "velo_graph_order: negative count");
    if (!perm || !first || !stats || (n_edges > 0 && (!a || !b))) return fail(VELO_ERR_INVALID, "velo_graph_order: null argument");
    for (int32_t e = 0; e < n_edges; e++) {
        if (a[e] < 0 || a[e] >= n_nodes || b[e] < 0 || b[e] >= n_nodes) return fail(VELO_ERR_INVALID, "velo_graph_order: edge %d joins %d and %d; nodes 0..%d", e, a[e], b[e], n_nodes - 1);
        if (a[e] == b[e]) return fail(VELO_ERR_INVALID, "velo_graph_order: edge %d: a == b (%d)", e, a[e]);
    }
    graph_order(n_nodes, n_edges, a, b, perm, first, stats);
    return VELO_OK;
}

int velo_graph_order_extend(int32_t n_old, const int32_t* perm_old, int32_t n_nodes, int32_t n_edges, const int32_t* a, const int32_t* b, int32_t first_new_edge,
                            int64_t max_work, int32_t* perm, int32_t* first, int64_t* stats) {
    const char* who = "velo_graph_order_extend";
    if (n_old < 0 || n_nodes < n_old || n_edges < 0) return fail(VELO_ERR_INVALID, "%s: counts must satisfy 0 <= n_old <= n_nodes and 0 <= n_edges", who);
    if (first_new_edge < 0 || first_new_edge > n_edges) return fail(VELO_ERR_INVALID, "%s: first_new_edge %d; 0..%d", who, first_new_edge, n_edges);
    if (max_work < 0) return fail(VELO_ERR_INVALID, "%s: negative max_work", who);
    if (!perm || !first || !stats || (n_old > 0 && !perm_old) || (n_edges > 0 && (!a || !b))) return fail(VELO_ERR_INVALID, "%s: null argument", who);
    std::vector<unsigned char> seen((size_t)n_old, 0);
    for (int32_t k = 0; k < n_old; k++) {
        if (perm_old[k] < 0 || perm_old[k] >= n_old || seen[(size_t)perm_old[k]]) return fail(VELO_ERR_INVALID, "%s: perm_old is not a permutation of 0..%d (entry %d is %d)", who, n_old - 1, k, perm_old[k]);
        seen[(size_t)perm_old[k]] = 1;
    }
    for (int32_t e = 0; e < n_edges; e++) {
        if (a[e] < 0 || a[e] >= n_nodes || b[e] < 0 || b[e] >= n_nodes) return fail(VELO_ERR_INVALID, "%s: edge %d joins %d and %d; nodes 0..%d", who, e, a[e], b[e], n_nodes - 1);
        if (a[e] == b[e]) return fail(VELO_ERR_INVALID, "%s: edge %d: a == b (%d)", who, e, a[e]);
        if (e < first_new_edge && (a[e] >= n_old || b[e] >= n_old)) return fail(VELO_ERR_INVALID, "%s: edge %d is not new (first_new_edge %d) and ends at a new node (%d, %d; n_old %d)", who, e, first_new_edge, a[e], b[e], n_old);
    }
    if (!graph_order_extend(n_old, perm_old, n_nodes, n_edges, a, b, first_new_edge, max_work, perm, first, stats))
        return fail(VELO_ERR_STATE, "%s: a row before the first dirty row does not keep its first column", who);
    return VELO_OK;
}

int velo_graph_retain(velo_ctx* c, const int32_t* fixed, int32_t n_fixed, const velo_graph_params* params, const int32_t* perm, int32_t n_perm) {
    const char* who = "velo_graph_retain";
    VELO_TRY(graph_check(c, fixed, n_fixed, params, who));
    if (perm && n_perm < 0) return fail(VELO_ERR_INVALID, "%s: negative n_perm", who);
    GraphStore& S = *c->graph;
    GraphRetained& R = S.ret;
    const int64_t max_work = graph_work_cap(params);
    HIP_TRY(hipSetDevice(c->device));
    const bool same = R.state != 0 && R.max_work == max_work && R.fixed.size() == (size_t)n_fixed && std::equal(R.fixed.begin(), R.fixed.end(), fixed);
    if (!perm && same && R.state == 1) return VELO_OK;                 // retained and current
    if (!perm && same) {                                               // behind: extended, as the next query would
        bool ok = false;
        VELO_TRY(graph_ret_extend(c, &ok));
        if (ok) return VELO_OK;
    }
    GraphCall call;
    call.who = who;
    VELO_TRY(graph_begin(c, fixed, n_fixed, graph_params(nullptr), &call));
    const size_t n = (size_t)call.n_free;
    // every refusal from here on leaves nothing retained; the order's arguments are checked before the state goes
    std::vector<int32_t> ea, eb, slot, order(n), first(n), ints;
    size_t m_seen = 0;
    graph_free_edges(S, call.free_nodes, S.n_edges, &ea, &eb, &m_seen, &slot);
    int64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int status = VELO_OK;
    if (perm) {
        std::vector<unsigned char> seen(n, 0);
        if ((size_t)n_perm != n) status = fail(VELO_ERR_INVALID, "%s: perm has %d entries; the graph has %zu free nodes", who, n_perm, n);
        for (size_t k = 0; k < n && status == VELO_OK; k++) {
            if (perm[k] < 0 || (size_t)perm[k] >= n || seen[(size_t)perm[k]]) status = fail(VELO_ERR_INVALID, "%s: perm is not a permutation of the free nodes' indices 0..%zu (entry %zu is %d)", who, n - 1, k, perm[k]);
            else seen[(size_t)perm[k]] = 1;
        }
        if (status == VELO_OK) {
            std::memcpy(order.data(), perm, sizeof(int32_t) * n);
            graph_first_of((int32_t)n, (int32_t)ea.size(), ea.data(), eb.data(), order.data(), first.data(), st);
        }
    } else if (!graph_order_extend(0, nullptr, (int32_t)n, (int32_t)ea.size(), ea.data(), eb.data(), 0, max_work, order.data(), first.data(), st))
        status = fail(VELO_ERR_STATE, "%s: the order's rule failed", who);
    if (status == VELO_OK) status = graph_env_refusal(who, st, max_work, n, "raise reserved[1]");
    if (status != VELO_OK) { (void)hipStreamSynchronize(c->stream); return status; }      // (refused on the host: a state retained before stays)
    graph_ret_drop(S);                                                 // the buffers are written from here on
    graph_env_ints(n, order.data(), first.data(), &ints);
    bool bad = false;
    GraphArgs A;
    VELO_TRY(graph_ret_factor(c, R, call, ints, st[1], -1, 0, &bad, &A));
    if (bad) return graph_cov_refuse(c, call.free_nodes, ints.data(), A, who);
    R.fixed.assign(fixed, fixed + n_fixed);
    R.max_work = max_work;
    graph_ret_commit(S, R, call, ints, st);
    R.counters[0]++;
    R.last_p = 0; R.last_rows = 0;
    return VELO_OK;
}

int velo_graph_release(velo_ctx* c) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    if (!c->graph) return VELO_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipStreamSynchronize(c->stream));           // nothing of the state is in flight when its buffers go
    c->graph->ret = GraphRetained();
    return VELO_OK;
}

int velo_graph_retained(velo_ctx* c, int64_t info[16], int32_t* perm_out, int32_t capacity) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    if (!info) return fail(VELO_ERR_INVALID, "velo_graph_retained: null info");
    if (capacity < 0 || (capacity > 0 && !perm_out)) return fail(VELO_ERR_INVALID, "velo_graph_retained: a negative capacity, or a null perm_out with a positive one");
    for (int k = 0; k < 16; k++) info[k] = 0;
    if (!c->graph) return VELO_OK;
    const GraphRetained& R = c->graph->ret;
    info[0] = R.state;
    if (R.state != 0) {
        info[1] = (int64_t)R.free_nodes.size(); info[2] = R.stats[0]; info[3] = R.stats[1]; info[4] = R.stats[2];
        const size_t m = std::min((size_t)capacity, R.free_nodes.size());
        if (m) std::memcpy(perm_out, R.ints.data(), sizeof(int32_t) * m);
    }
    for (int k = 0; k < 6; k++) info[5 + k] = R.counters[k];
    info[11] = R.last_p; info[12] = R.last_rows;
    return VELO_OK;
}

int velo_graph_system(velo_ctx* c, const int32_t* fixed, int32_t n_fixed, double* cost, double* gradient, double* diag_blocks) {
    VELO_TRY(graph_check(c, fixed, n_fixed, nullptr, "velo_graph_system"));
    GraphStore& S = *c->graph;
    GraphCall call;
    VELO_TRY(graph_begin(c, fixed, n_fixed, graph_params(nullptr), &call));
    const size_t n = (size_t)call.n_free;
    unsigned char* tail = S.h_out.p + sizeof(GraphRecord);
    if (n) HIP_TRY(hipMemcpyAsync(tail, S.nd.p, sizeof(double) * n * kGrNode, hipMemcpyDeviceToHost, c->stream));   // the state starts in buffer 0
    GraphRecord* rec = nullptr;
    VELO_TRY(graph_read_record(c, S, &rec));
    if (cost) *cost = rec->red[0];
    const double* nd = (const double*)tail;
    for (size_t i = 0; i < n; i++) expand_upper6(nd + i * kGrNode, gradient ? gradient + 6 * i : nullptr, diag_blocks ? diag_blocks + 36 * i : nullptr);
    return VELO_OK;
}

int velo_graph_covariance(velo_ctx* c, const int32_t* fixed, int32_t n_fixed, const velo_graph_params* params, int32_t n_pairs,
                          const int32_t* frame_a, const int32_t* frame_b, double* cov36) {
    const char* who = "velo_graph_covariance";
    VELO_TRY(graph_check(c, fixed, n_fixed, params, who));
    if (n_pairs < 0) return fail(VELO_ERR_INVALID, "%s: negative pair count", who);
    if (n_pairs > 0 && (!frame_a || !frame_b || !cov36)) return fail(VELO_ERR_INVALID, "%s: null pair array or output", who);
    GraphStore& S = *c->graph;
    for (int p = 0; p < n_pairs; p++) {
        const int32_t ends[2] = {frame_a[p], frame_b[p]};
        for (int k = 0; k < 2; k++) {
            VELO_TRY(check_frame(ends[k], who, p));
            if (!graph_has_pose(S, ends[k])) return fail(VELO_ERR_STATE, "%s: pair %d names frame %d, which has no pose", who, p, ends[k]);
        }
    }
    if (n_pairs == 0) return VELO_OK;
    GraphFactor Q;
    VELO_TRY(graph_query_open(c, fixed, n_fixed, params, who, &Q));
    const size_t np = (size_t)n_pairs;
    // per pair: the free indices of its ends (-1: a constant) and, for a pair outside the envelope, the slot of its column solve
    std::vector<int32_t> pr(3 * np);
    size_t n_out = 0;
    for (size_t p = 0; p < np; p++) {
        const int32_t ia = Q.free_index(frame_a[p]), ib = Q.free_index(frame_b[p]);
        pr[3 * p] = ia; pr[3 * p + 1] = ib; pr[3 * p + 2] = ia >= 0 && ib >= 0 && Q.outside(ia, ib) ? (int32_t)n_out++ : -1;
    }
    VELO_TRY(graph_query_reserve(c, &Q, who, "pairs outside the envelope", kGraphRecDoubles + 36 * np, n_out, nullptr, nullptr));
    VELO_TRY(S.cov_pair.reserve(3 * np));
    VELO_TRY(S.in_ev.wait_or_create());
    VELO_TRY(S.h_in.reserve(sizeof(int32_t) * 3 * np));
    std::memcpy(S.h_in.p, pr.data(), sizeof(int32_t) * 3 * np);
    HIP_TRY(hipMemcpyAsync(S.cov_pair.p, S.h_in.p, sizeof(int32_t) * 3 * np, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(S.in_ev, c->stream));
    GraphCov V;
    V.zenv = Q.zenv; V.work = Q.work; V.pair = S.cov_pair.p; V.out = S.cov_out.p + kGraphRecDoubles; V.n_pairs = n_pairs;
    VELO_TRY(graph_query_enqueue(c, Q, &V, nullptr));
    if (n_out) hipLaunchKernelGGL(graph_env_column_kernel, dim3((unsigned)n_out), dim3(kGrEnvColumnThreads), 0, c->stream, Q.A, V);
    hipLaunchKernelGGL(graph_cov_gather_kernel, dim3((unsigned)np), dim3(64), 0, c->stream, Q.A, V);
    VELO_TRY(graph_query_finish(c, Q, who));
    std::memcpy(cov36, S.h_out.p + sizeof(GraphRecord), sizeof(double) * 36 * np);
    return VELO_OK;
}

int velo_graph_edge_gate(velo_ctx* c, const int32_t* fixed, int32_t n_fixed, const velo_graph_params* params, int32_t n_pairs,
                         const int32_t* from, const int32_t* to, const double* z, const double* info21,
                         double* rel6, double* r6, double* cov36, double* chi2) {
    const char* who = "velo_graph_edge_gate";
    VELO_TRY(graph_check(c, fixed, n_fixed, params, who));
    if (n_pairs < 0) return fail(VELO_ERR_INVALID, "%s: negative pair count", who);
    if (n_pairs > 0 && (!from || !to)) return fail(VELO_ERR_INVALID, "%s: null pair array", who);
    GraphStore& S = *c->graph;
    const size_t np = (size_t)std::max(n_pairs, 0);
    std::vector<double> L(info21 ? 21 * np : 0);
    for (int p = 0; p < n_pairs; p++) {
        if (from[p] < 0 || from[p] >= kLmMaxFrame || to[p] < 0 || to[p] >= kLmMaxFrame) return fail(VELO_ERR_INVALID, "%s: pair %d: frames %d -> %d; 0..%d", who, p, from[p], to[p], kLmMaxFrame - 1);
        if (from[p] == to[p]) return fail(VELO_ERR_INVALID, "%s: pair %d: from == to (%d)", who, p, from[p]);
        const int32_t ends[2] = {from[p], to[p]};
        for (int k = 0; k < 2; k++)
            if (!graph_has_pose(S, ends[k])) return fail(VELO_ERR_STATE, "%s: pair %d names frame %d, which has no pose", who, p, ends[k]);
        for (int k = 0; z && k < 6; k++) if (!std::isfinite(z[6 * (size_t)p + k])) return fail(VELO_ERR_INVALID, "%s: pair %d: z[%d] is not finite", who, p, k);
        if (info21) {                                                  // as velo_graph_add_edges_weighted validates an edge's
            const double* u = info21 + 21 * (size_t)p;
            for (int k = 0; k < 21; k++) if (!std::isfinite(u[k])) return fail(VELO_ERR_INVALID, "%s: pair %d: info21[%d] is not finite", who, p, k);
            if (!graph_host_chol6(u, L.data() + 21 * (size_t)p))
                return fail(VELO_ERR_INVALID, "%s: pair %d: its information matrix is not positive definite (the Cholesky factorisation met a pivot that is not positive and finite)", who, p);
        }
    }
    if (n_pairs == 0) return VELO_OK;
    GraphFactor Q;
    VELO_TRY(graph_query_open(c, fixed, n_fixed, params, who, &Q));
    // per pair: its frames, their free indices and, for a pair outside the envelope, the slot of the full column of one end -- `to`'s; the
    // pairs that share that frame share the column
    std::vector<int32_t> pr(5 * np), col_of(Q.n, -1), cols, remap;
    for (size_t p = 0; p < np; p++) {
        const int32_t ia = Q.free_index(from[p]), ib = Q.free_index(to[p]);
        int32_t slot = -1;
        if (ia >= 0 && ib >= 0 && Q.outside(ia, ib)) {
            if (col_of[(size_t)ib] < 0) { col_of[(size_t)ib] = (int32_t)cols.size(); cols.push_back(Q.pos[(size_t)ib]); }
            slot = col_of[(size_t)ib];
        }
        int32_t* q = pr.data() + 5 * p;
        q[0] = from[p]; q[1] = to[p]; q[2] = ia; q[3] = ib; q[4] = slot;
    }
    const size_t nc = cols.size(), n_ints = 5 * np + nc, n_dbl = (z ? 6 * np : 0) + 21 * (info21 ? np : 0);
    VELO_TRY(graph_query_reserve(c, &Q, who, "block columns", kGraphRecDoubles + kGrRelOut * np, 0, &cols, &remap));
    for (size_t p = 0; p < np; p++) if (pr[5 * p + 4] >= 0) pr[5 * p + 4] = remap[(size_t)pr[5 * p + 4]];      // (a retained state keeps its column in slot 0)
    VELO_TRY(S.rel_i.reserve(n_ints));
    VELO_TRY(S.rel_d.reserve(n_dbl + 1));
    VELO_TRY(S.in_ev.wait_or_create());
    VELO_TRY(S.h_in.reserve(sizeof(double) * n_dbl + sizeof(int32_t) * n_ints));
    double* hd = (double*)S.h_in.p;                                    // z, then L, then the ints
    int32_t* hi = (int32_t*)(hd + n_dbl);
    if (z) std::memcpy(hd, z, sizeof(double) * 6 * np);
    if (info21) std::memcpy(hd + (z ? 6 * np : 0), L.data(), sizeof(double) * 21 * np);
    std::memcpy(hi, pr.data(), sizeof(int32_t) * 5 * np);
    if (nc) std::memcpy(hi + 5 * np, cols.data(), sizeof(int32_t) * nc);
    if (n_dbl) HIP_TRY(hipMemcpyAsync(S.rel_d.p, hd, sizeof(double) * n_dbl, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(S.rel_i.p, hi, sizeof(int32_t) * n_ints, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(S.in_ev, c->stream));
    GraphRel R;
    R.zenv = Q.zenv; R.work = Q.work; R.col_pos = S.rel_i.p + 5 * np; R.pair = S.rel_i.p;
    R.z = z ? S.rel_d.p : nullptr; R.linfo = info21 ? S.rel_d.p + (z ? 6 * np : 0) : nullptr;
    R.out = S.cov_out.p + kGraphRecDoubles; R.n_pairs = n_pairs;
    VELO_TRY(graph_query_enqueue(c, Q, nullptr, &R));
    hipLaunchKernelGGL(graph_relcov_kernel, dim3((unsigned)np), dim3(64), 0, c->stream, Q.A, R);
    VELO_TRY(graph_query_finish(c, Q, who));
    const double* res = (const double*)S.h_out.p + kGraphRecDoubles;
    for (size_t p = 0; p < np; p++) {
        const double* o = res + kGrRelOut * p;
        if (rel6) std::memcpy(rel6 + 6 * p, o, sizeof(double) * 6);
        if (r6) std::memcpy(r6 + 6 * p, o + 6, sizeof(double) * 6);
        if (cov36) std::memcpy(cov36 + 36 * p, o + 12, sizeof(double) * 36);
        if (chi2) chi2[p] = o[48];
    }
    return VELO_OK;
}

int velo_graph_loop_candidates(velo_ctx* c, const int32_t* fixed, int32_t n_fixed, const velo_graph_params* params, int32_t query, int32_t min_gap,
                               double radius, double k_sigma, int32_t capacity, int32_t* frames_out, double* dist_out, double* sigma_out, int32_t* n_found) {
    const char* who = "velo_graph_loop_candidates";
    VELO_TRY(graph_check(c, fixed, n_fixed, params, who));
    VELO_TRY(check_frame(query, who));
    if (min_gap < 1) return fail(VELO_ERR_INVALID, "%s: min_gap %d; at least 1", who, min_gap);
    if (!(radius >= 0.0) || !std::isfinite(radius)) return fail(VELO_ERR_INVALID, "%s: radius must be non-negative and finite", who);
    if (!(k_sigma >= 0.0) || !std::isfinite(k_sigma)) return fail(VELO_ERR_INVALID, "%s: k_sigma must be non-negative and finite", who);
    if (capacity < 0) return fail(VELO_ERR_INVALID, "%s: negative capacity", who);
    if (!n_found) return fail(VELO_ERR_INVALID, "%s: null n_found", who);
    GraphStore& S = *c->graph;
    if (!graph_has_pose(S, query)) return fail(VELO_ERR_STATE, "%s: the query frame %d has no pose", who, query);
    const size_t F = S.frame_cap;
    const bool with_sigma = k_sigma > 0.0;
    GraphFactor Q;
    if (with_sigma) VELO_TRY(graph_query_open(c, fixed, n_fixed, params, who, &Q));
    else {                                                             // distances alone: the stored poses to buffer 0, no system
        HIP_TRY(hipSetDevice(c->device));
        VELO_TRY(S.x.reserve(2 * F * 6 + 1));
        HIP_TRY(hipMemcpyAsync(S.x.p, S.h_x.p, sizeof(double) * F * 6, hipMemcpyHostToDevice, c->stream));
        Q.A.x = S.x.p; Q.A.x_stride = F * 6;
    }
    // per frame: -2 = no pose, -1 = a constant, otherwise the free index; without sigma only `no pose` matters
    std::vector<int32_t> slot(F, -2);
    for (size_t f = 0; f < F; f++) if (S.pose_set[f]) slot[f] = -1;
    for (size_t i = 0; i < Q.n; i++) slot[(size_t)(*Q.free_nodes)[i]] = (int32_t)i;
    const int32_t iq = with_sigma ? slot[(size_t)query] : -1;
    std::vector<int32_t> cols(iq >= 0 ? 1 : 0, iq >= 0 ? Q.pos[(size_t)iq] : 0), remap;      // the query's full column
    const size_t cap = std::min((size_t)capacity, F);
    VELO_TRY(graph_query_reserve(c, &Q, who, "block columns", kGraphRecDoubles + 1 + 3 * cap, 0, &cols, &remap));
    VELO_TRY(S.rel_i.reserve(2 * F + 1));
    VELO_TRY(S.rel_d.reserve(2 * F + 1));
    VELO_TRY(S.in_ev.wait_or_create());
    VELO_TRY(S.h_in.reserve(sizeof(int32_t) * (F + 1)));
    int32_t* hi = (int32_t*)S.h_in.p;                                  // the slots, then the position of the query's column
    std::memcpy(hi, slot.data(), sizeof(int32_t) * F);
    hi[F] = cols.empty() ? 0 : cols[0];
    HIP_TRY(hipMemcpyAsync(S.rel_i.p, hi, sizeof(int32_t) * (F + 1), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(S.in_ev, c->stream));
    GraphRel R;
    std::memset(&R, 0, sizeof(R));
    R.zenv = Q.zenv; R.work = Q.work; R.col_pos = S.rel_i.p + F;
    GraphCand K;
    K.zenv = Q.zenv; K.work = Q.work; K.slot = S.rel_i.p; K.flag = S.rel_i.p + F + 1; K.rec = S.rel_d.p;
    K.out = S.cov_out.p + kGraphRecDoubles;
    K.n_frames = (int)F; K.query = query; K.min_gap = min_gap; K.capacity = (int)cap; K.with_sigma = with_sigma ? 1 : 0;
    K.radius = radius; K.k_sigma = k_sigma;
    VELO_TRY(graph_query_enqueue(c, Q, nullptr, &R));
    hipLaunchKernelGGL(graph_loop_candidates_kernel, dim3((unsigned)cdiv((int)F, kGrThreads)), dim3(kGrThreads), 0, c->stream, Q.A, K);
    hipLaunchKernelGGL(graph_loop_compact_kernel, dim3(1), dim3(kGrCompactThreads), 0, c->stream, K);
    VELO_TRY(graph_query_finish(c, Q, who));
    const double* res = (const double*)S.h_out.p + kGraphRecDoubles;
    const size_t found = (size_t)res[0];
    for (size_t k = 0; k < std::min(found, cap); k++) {
        if (frames_out) frames_out[k] = (int32_t)res[1 + 3 * k];
        if (dist_out) dist_out[k] = res[2 + 3 * k];
        if (sigma_out) sigma_out[k] = res[3 + 3 * k];
    }
    *n_found = (int32_t)found;
    return VELO_OK;
}

int velo_graph_optimize(velo_ctx* c, const int32_t* fixed, int32_t n_fixed, const velo_graph_params* params, velo_graph_summary* summary) {
    VELO_TRY(graph_check(c, fixed, n_fixed, params, "velo_graph_optimize"));
    GraphStore& S = *c->graph;
    const velo_graph_params P = graph_params(params);
    GraphCall call;
    call.envelope = P.reserved[0] == VELO_GRAPH_SOLVER_ENVELOPE;
    call.max_work = graph_work_cap(&P);
    VELO_TRY(graph_begin(c, fixed, n_fixed, P, &call));
    graph_ret_drop(S);                                                 // a solve that runs ends a retained factorisation, whatever its outcome
    const GraphArgs& A = call.A;
    const LMParams Q = A.lm;
    const int n = call.n_free, E = call.E, nb = A.nb;
    const int cg_cap = P.cg_max_iterations;
    const bool envelope = call.envelope;
    velo_graph_summary sum;
    std::memset(&sum, 0, sizeof(sum));
    sum.n_nodes = S.n_nodes; sum.n_free = n; sum.n_edges = E;
    GraphRecord* rec = nullptr;
    VELO_TRY(graph_read_record(c, S, &rec));
    TrustRegion T;                                                     // B1, on the host (velo_trust_region.h)
    tr_start(Q, &T, rec->red[0], std::sqrt(rec->red[3]), rec->red[4]);
    sum.initial_cost = T.cost;
    if (n == 0 || E == 0) tr_stop(&T, VELO_CONVERGENCE);
    int cur = 0;
    const unsigned g_nodes = (unsigned)nb;
    while (!T.done && !tr_head(Q, &T)) {
        // the linear step: the envelope's fill, factor, solve and one record; or CG in batches, one record per batch
        HIP_TRY(hipMemsetAsync(S.rec.p, 0, sizeof(GraphRecord), c->stream));
        int k = 0, batch = 32;
        if (envelope) {
            hipLaunchKernelGGL(graph_env_fill_kernel, dim3((unsigned)n), dim3(64), 0, c->stream, A, cur, T.radius, T.refresh);
            hipLaunchKernelGGL(graph_env_factor_kernel, dim3(1), dim3(kGrEnvFactorThreads), 0, c->stream, A);
            hipLaunchKernelGGL(graph_env_solve_kernel, dim3(1), dim3(kGrEnvSolveThreads), 0, c->stream, A, cur);
            HIP_TRY(hipGetLastError());
            VELO_TRY(graph_read_record(c, S, &rec));
        } else hipLaunchKernelGGL(graph_cg_begin_kernel, dim3(g_nodes), dim3(kGrThreads), 0, c->stream, A, cur, T.radius, T.refresh);
        while (!envelope && k < cg_cap) {
            const int m = std::min(batch, cg_cap - k);
            for (int j = 0; j < m; j++) {
                hipLaunchKernelGGL(graph_cg_ap_kernel, dim3(g_nodes), dim3(kGrThreads), 0, c->stream, A, k + j, cur, T.radius);
                hipLaunchKernelGGL(graph_cg_update_kernel, dim3(g_nodes), dim3(kGrThreads), 0, c->stream, A, k + j);
            }
            k += m;
            HIP_TRY(hipGetLastError());
            VELO_TRY(graph_read_record(c, S, &rec));
            if (rec->cg_done) break;
            batch = std::min(2 * batch, 256);
        }
        bool ok = rec->bad == 0;
        if (ok) {                                                      // the candidate, linearised and reduced
            hipLaunchKernelGGL(graph_step_kernel, dim3(g_nodes), dim3(kGrThreads), 0, c->stream, A, k, cur);
            graph_linearize(c, A, call.W, cur ^ 1);
            hipLaunchKernelGGL(graph_assemble_kernel, dim3(g_nodes), dim3(kGrThreads), 0, c->stream, A, cur ^ 1, 1);
            hipLaunchKernelGGL(graph_reduce_kernel, dim3(kGrRed), dim3(256), 0, c->stream, A, cur ^ 1);
            HIP_TRY(hipGetLastError());
            VELO_TRY(graph_read_record(c, S, &rec));
            ok = rec->red[1] > 0.0 && std::isfinite(rec->red[1]);
        }
        velo_graph_iteration t;
        std::memset(&t, 0, sizeof(t));
        t.iteration = T.iteration; t.cost = T.cost; t.radius = T.radius; t.cg_iterations = rec->cg_iters; t.cg_residual = rec->cg_rel;
        if (!ok) t.status = tr_invalid(Q, &T);
        else {
            t.candidate_cost = rec->red[0]; t.model_change = rec->red[1]; t.step_norm = std::sqrt(rec->red[2]);
            t.status = tr_candidate(Q, &T, t.candidate_cost, t.model_change, t.step_norm);
            if (t.status == VELO_BA_ACCEPTED) { cur ^= 1; t.status = tr_accept(Q, &T, std::sqrt(rec->red[3]), rec->red[4]); }
        }
        if (sum.n_trace < VELO_GRAPH_MAX_TRACE) sum.trace[sum.n_trace++] = t;
    }
    sum.termination = T.termination; sum.iterations = T.iteration; sum.evaluations = T.evaluations; sum.final_cost = T.cost;
    if (T.n_accepted > 0) {                                            // parameters move on accepted steps only
        double* back = (double*)(S.h_out.p + sizeof(GraphRecord));
        HIP_TRY(hipMemcpyAsync(back, S.x.p + (size_t)cur * A.x_stride, sizeof(double) * A.x_stride, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        for (int i = 0; i < n; i++) std::memcpy(S.h_x.p + (size_t)call.free_nodes[(size_t)i] * 6, back + (size_t)call.free_nodes[(size_t)i] * 6, sizeof(double) * 6);
    }
    S.n_optimized++;
    if (envelope) { S.env_widest = (int)call.env_stats[0]; S.env_blocks = (int)call.env_stats[1]; }
    if (summary) *summary = sum;
    return VELO_OK;
}

}  // extern "C"
