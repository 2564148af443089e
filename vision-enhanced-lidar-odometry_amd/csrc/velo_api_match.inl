// velo_api_match.inl -- part of the host side of the C-ABI, included by velo_hip.hip (ONE translation unit; the order of the parts is the order of
// definition).  C-ABI: batched Hamming matching of 64-byte descriptors -- matchFeatures (velo.h:499-560); kernels in velo_match_kernels.h.
extern "C" {   // (continued from the previous part)
int velo_match_descriptors(velo_ctx* c, const velo_desc_job* jobs, int32_t n_jobs, double match_thresh, int32_t* train_idx, int32_t* distance,
                           int32_t* min_dist, int32_t* n_kept, int32_t* pairs) {
    // every argument is checked before the context is touched
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    if (n_jobs < 0) return fail(VELO_ERR_INVALID, "negative job count %d", n_jobs);
    if (n_jobs == 0) return VELO_OK;
    if (!jobs || !min_dist || !n_kept) return fail(VELO_ERR_INVALID, "null jobs / min_dist / n_kept");
    if (std::isnan(match_thresh)) return fail(VELO_ERR_INVALID, "match_thresh is NaN");
    int64_t total_q = 0;
    for (int j = 0; j < n_jobs; j++) {
        const velo_desc_job& J = jobs[j];
        if (J.n_query < 0 || J.n_train < 0) return fail(VELO_ERR_INVALID, "job %d: negative size (%d queries, %d train rows)", j, J.n_query, J.n_train);
        if ((J.n_query > 0 && !J.query) || (J.n_train > 0 && !J.train)) return fail(VELO_ERR_INVALID, "job %d: null descriptor rows", j);
        if (J.n_train > kMatchMaxRows) return fail(VELO_ERR_INVALID, "job %d: %d train rows; the match key indexes at most %d", j, J.n_train, kMatchMaxRows);
        total_q += J.n_query;
    }
    if (total_q > (int64_t)(INT32_MAX / 4)) return fail(VELO_ERR_INVALID, "%lld queries in one call; at most %d", (long long)total_q, INT32_MAX / 4);
    if (total_q > 0 && (!train_idx || !distance || !pairs)) return fail(VELO_ERR_INVALID, "null train_idx / distance / pairs");

    // the distinct sets of the call, each staged once: (pointer, rows) -> first row in the upload
    std::vector<MatchJob> hj((size_t)n_jobs);
    std::unordered_map<const uint8_t*, std::vector<std::pair<int, int>>> first_row;   // pointer -> (rows, first row)
    std::vector<std::pair<const uint8_t*, int>> sets;
    int64_t n_rows = 0;
    auto stage = [&](const uint8_t* p, int n) -> int {
        if (n == 0) return 0;
        for (const auto& e : first_row[p]) if (e.first == n) return e.second;
        const int r = (int)n_rows;
        first_row[p].emplace_back(n, r);
        sets.emplace_back(p, n);
        n_rows += n;
        return r;
    };
    const bool valu = c->match_variant == 0;
    const int tq = valu ? kMatchValuQ : kMatchQ, tt = valu ? kMatchValuT : kMatchT;
    int64_t blocks = 0, q_out = 0;
    for (int j = 0; j < n_jobs; j++) {
        const velo_desc_job& J = jobs[j];
        MatchJob& M = hj[(size_t)j];
        std::memset(&M, 0, sizeof(M));
        M.q_row = stage(J.query, J.n_query);
        M.t_row = stage(J.train, J.n_train);
        if (n_rows > (int64_t)INT32_MAX / 4) return fail(VELO_ERR_INVALID, "more than %d distinct descriptor rows in one call", INT32_MAX / 4);
        M.n_query = J.n_query; M.n_train = J.n_train;
        M.q_out = (int)q_out;
        M.blk_start = (int)blocks;
        M.nqb = cdiv(J.n_query, tq);
        if (J.n_query > 0 && J.n_train > 0) blocks += (int64_t)M.nqb * cdiv(J.n_train, tt);
        if (blocks > (int64_t)INT32_MAX) return fail(VELO_ERR_INVALID, "too many match blocks in one call");
        q_out += J.n_query;
    }
    const int nq = (int)total_q;

    HIP_TRY(hipSetDevice(c->device));
    StageLayout in;
    const auto mjobs = in.add<MatchJob>((size_t)n_jobs);
    const auto rows = in.add<uint4>(4 * (size_t)n_rows);                       // the rows start 64-byte aligned
    const size_t out_ints = 4 * (size_t)nq + 2 * (size_t)n_jobs;               // the filter kernel's own layout: one part
    VELO_TRY(c->md_in.reserve(in.bytes));
    VELO_TRY(c->h_md_out.reserve(sizeof(int) * out_ints));
    VELO_TRY(c->md_keys.reserve((size_t)nq + (size_t)n_jobs));
    VELO_TRY(c->md_out.reserve(out_ints));
    std::memcpy(mjobs.in(c->md_in.h.p), hj.data(), mjobs.size());
    {
        unsigned char* w = (unsigned char*)rows.in(c->md_in.h.p);
        for (const auto& s : sets) { std::memcpy(w, s.first, 64 * (size_t)s.second); w += 64 * (size_t)s.second; }
    }
    HIP_TRY(hipMemcpyAsync(c->md_in.d.p, c->md_in.h.p, in.bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->md_keys.p, 0xFF, sizeof(unsigned) * ((size_t)nq + (size_t)n_jobs), c->stream));   // kMatchNone
    const MatchJob* djobs = mjobs.in(c->md_in.d.p);
    const uint4* drows = rows.in(c->md_in.d.p);
    unsigned* keys = c->md_keys.p;
    unsigned* dmin = c->md_keys.p + nq;
    if (blocks > 0) {
        if (valu)
            hipLaunchKernelGGL(match_valu_kernel, dim3((unsigned)blocks), dim3(kMatchThreads), 0, c->stream, drows, djobs, n_jobs, keys, dmin);
        else
            hipLaunchKernelGGL(match_mfma_kernel, dim3((unsigned)blocks), dim3(kMatchThreads), 0, c->stream, drows, djobs, n_jobs, keys, dmin);
    }
    hipLaunchKernelGGL(match_filter_kernel, dim3(n_jobs), dim3(kMatchThreads), 0, c->stream, djobs, (const unsigned*)keys, (const unsigned*)dmin,
                       match_thresh, nq, c->md_out.p);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_md_out.p, c->md_out.p, sizeof(int) * out_ints, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));

    const int* o = c->h_md_out.p;
    if (nq > 0) {
        std::memcpy(train_idx, o, sizeof(int) * (size_t)nq);
        std::memcpy(distance, o + nq, sizeof(int) * (size_t)nq);
    }
    int64_t w = 0;
    for (int j = 0; j < n_jobs; j++) {
        min_dist[j] = o[4 * (size_t)nq + 2 * (size_t)j];
        n_kept[j] = o[4 * (size_t)nq + 2 * (size_t)j + 1];
        if (n_kept[j] > 0) std::memcpy(pairs + 2 * w, o + 2 * (size_t)nq + 2 * (size_t)hj[(size_t)j].q_out, sizeof(int) * 2 * (size_t)n_kept[j]);
        w += n_kept[j];
    }
    return VELO_OK;
}

}  // extern "C"
