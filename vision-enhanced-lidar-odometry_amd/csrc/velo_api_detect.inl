// velo_api_detect.inl -- part of the host side of the C-ABI, included by velo_hip.hip (ONE translation unit; the order of the parts is the order of
// definition).  C-ABI: GFTT corner detection on the current resident images (velo_detect_features[_batch]: detectFeatures,
// velo.h:118-177; velo_get_corner_response); kernels in velo_detect_kernels.h.  One implementation over a list of contexts, which the
// single-context entry hands a list of one (velo_api_track.inl says who lends what; the staged tables are laid out by a StageLayout).
namespace {

constexpr int kGfDetectUnits = 64;         // cameras per detection launch set (a call with more runs in chunks)

inline float gf_scale2() {                 // cornerMinEigenVal: 1 / (255 * 2^(ksize - 1) * blockSize), squared
    const float s = (float)(1.0 / (255.0 * 4.0 * 3.0));
    return s * s;
}

// the argument checks of detection that read no context
int gf_check_params(int32_t n_jobs, const velo_gftt_params* p, int32_t capacity) {
    if (n_jobs < 0) return fail(VELO_ERR_INVALID, "negative job count %d", n_jobs);
    if (!p) return fail(VELO_ERR_INVALID, "null params");
    if (p->block_size != 3) return fail(VELO_ERR_INVALID, "block_size %d; only 3 is supported", p->block_size);
    if (!(p->min_distance >= 1.0 && p->min_distance <= (double)kGfMaxDist))
        return fail(VELO_ERR_INVALID, "min_distance %g; 1..%d", p->min_distance, kGfMaxDist);
    if (!(p->quality_level > 0.0 && p->quality_level <= 1.0)) return fail(VELO_ERR_INVALID, "quality_level %g; (0, 1]", p->quality_level);
    if (capacity < 0) return fail(VELO_ERR_INVALID, "negative capacity %d", capacity);
    return VELO_OK;
}

// n_jobs > 0: the job list and the output arrays; *total = existing points of the call
int gf_check_jobs(const velo_detect_job* jobs, int32_t n_jobs, int32_t capacity, const float* xy, const float* response, const uint8_t* fresh,
                  const int32_t* counts, int64_t* total) {
    if (!jobs) return fail(VELO_ERR_INVALID, "null jobs");
    if (!counts) return fail(VELO_ERR_INVALID, "null counts");
    if (capacity > 0 && (!xy || !response || !fresh)) return fail(VELO_ERR_INVALID, "null xy / response / fresh");
    *total = 0;
    for (int j = 0; j < n_jobs; j++) {
        if (jobs[j].n_existing < 0) return fail(VELO_ERR_INVALID, "job %d: negative point count %d", j, jobs[j].n_existing);
        if (jobs[j].n_existing > 0 && !jobs[j].existing_xy) return fail(VELO_ERR_INVALID, "job %d: null points", j);
        VELO_TRY(check_cam(jobs[j].cam, kLkMaxCams, "job", j));
        *total += jobs[j].n_existing;
    }
    if (n_jobs > 4096) return fail(VELO_ERR_INVALID, "%d jobs in one call; at most 4096", n_jobs);
    if (*total > (int64_t)(INT32_MAX / 16)) return fail(VELO_ERR_INVALID, "%lld points in one call; at most %d", (long long)*total, INT32_MAX / 16);
    return VELO_OK;
}

// one launch set of detection: the units [u0, u0 + nu) of the call and the jobs `sel` that name them (call order)
struct GfUnitRef { int ctx, cam; };
int gf_run(velo_ctx** ctxs, int n_ctx, const std::vector<GfUnitRef>& units, int u0, int nu, const std::vector<int>& unit_of_job, const std::vector<int>& sel,
           const velo_detect_job* jobs, const velo_gftt_params* p, int32_t capacity, float* xy, float* response, uint8_t* fresh, int32_t* counts) {
    velo_ctx* c = ctxs[0];
    const int nj = (int)sel.size();
    // every unit's share of the scratch buffers: sizes differ, so offsets are summed, not multiplied
    std::vector<size_t> plane(nu), splane(nu), kcap(nu), o_plane(nu), o_state(nu), o_keys(nu);
    std::vector<int> sstride(nu);
    size_t t_plane = 0, t_state = 0, t_keys = 0, max_plane = 0;
    int max_w = 0, max_h = 0;
    for (int u = 0; u < nu; u++) {
        const LkSlot& S = *lk_slot(ctxs[units[u0 + u].ctx], false);
        plane[u] = (size_t)S.w * S.h;
        sstride[u] = (S.w + 2 * kGfStatePad + 3) & ~3;
        splane[u] = (size_t)sstride[u] * (S.h + 2 * kGfStatePad);
        kcap[u] = 1;
        while (kcap[u] < plane[u]) kcap[u] <<= 1;
        o_plane[u] = t_plane; o_state[u] = t_state; o_keys[u] = t_keys;
        t_plane += plane[u]; t_state += splane[u]; t_keys += kcap[u];
        max_plane = std::max(max_plane, plane[u]);
        max_w = std::max(max_w, S.w); max_h = std::max(max_h, S.h);
    }
    const int cap_d = (int)std::min<size_t>((size_t)capacity, max_plane);     // a camera has at most one corner per pixel
    VELO_TRY(c->gf_eig.reserve(t_plane));
    VELO_TRY(c->gf_state.reserve(t_state));
    VELO_TRY(c->gf_cand.reserve(2 * t_plane));
    VELO_TRY(c->gf_keys.reserve(t_keys));
    VELO_TRY(c->gf_hdr.reserve((size_t)kGfHdrStride * nu));
    GfParams K;
    std::memset(&K, 0, sizeof(K));
    K.scale2 = gf_scale2();
    K.radius = (int)std::ceil(p->min_distance) - 1;
    K.max_corners = p->max_corners;
    K.capacity = cap_d;
    K.quality = p->quality_level;
    K.md2 = p->min_distance * p->min_distance;
    K.md2f = (float)(p->min_distance * p->min_distance);
    int64_t total = 0;
    for (int k = 0; k < nj; k++) total += jobs[sel[k]].n_existing;
    const size_t n_slots = (size_t)nj * cap_d;
    StageLayout in, out;
    const auto gunits = in.add<GfUnit>((size_t)nu);
    const auto gjobs = in.add<GfJob>((size_t)nj);
    const auto have = in.add<float2>((size_t)total);
    const auto cnt = out.add<int>(3 * (size_t)nj);
    const auto oxy = out.add<float2>(n_slots);                   // on the line behind the counts; response and fresh packed behind it
    const auto oresp = out.add<float>(n_slots, 4);
    const auto ofresh = out.add<unsigned char>(n_slots, 1);
    VELO_TRY(c->gf_in.reserve(in.bytes));
    VELO_TRY(c->gf_out.reserve(out.bytes));
    {
        GfUnit* hu = gunits.in(c->gf_in.h.p);
        for (int u = 0; u < nu; u++) {
            const LkSlot& S = *lk_slot(ctxs[units[u0 + u].ctx], false);
            GfUnit& U = hu[u];
            U.plane = S.pix.p + (size_t)units[u0 + u].cam * S.cam_pix + S.pyr.lv[0].off;
            U.eig = c->gf_eig.p + o_plane[u];
            U.state = c->gf_state.p + o_state[u];
            U.cand = c->gf_cand.p + o_plane[u];
            U.und = c->gf_cand.p + t_plane + o_plane[u];
            U.keys = c->gf_keys.p + o_keys[u];
            U.hdr = c->gf_hdr.p + (size_t)u * kGfHdrStride;
            U.w = S.w; U.h = S.h; U.stride = S.pyr.lv[0].stride; U.sstride = sstride[u];
        }
        GfJob* hj = gjobs.in(c->gf_in.h.p);
        float* hp = (float*)have.in(c->gf_in.h.p);
        int first = 0;
        for (int k = 0; k < nj; k++) {
            const velo_detect_job& J = jobs[sel[k]];
            hj[k].unit = unit_of_job[sel[k]] - u0; hj[k].first = first; hj[k].n = J.n_existing; hj[k].pad_ = 0;
            if (J.n_existing > 0) std::memcpy(hp + 2 * (size_t)first, J.existing_xy, sizeof(float) * 2 * (size_t)J.n_existing);
            first += J.n_existing;
        }
    }
    std::vector<char> used(n_ctx, 0);
    for (int u = 0; u < nu; u++) used[units[u0 + u].ctx] = 1;
    VELO_TRY(fb_gather(ctxs, n_ctx, &used));
    HIP_TRY(hipMemcpyAsync(c->gf_in.d.p, c->gf_in.h.p, in.bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->gf_hdr.p, 0, sizeof(int) * kGfHdrStride * (size_t)nu, c->stream));
    HIP_TRY(hipMemsetAsync(c->gf_state.p, 0, t_state, c->stream));                          // the zero border of the state maps
    HIP_TRY(hipMemsetAsync(c->gf_out.d.p, 0, oxy.off, c->stream));                          // the counts, up to the line xy starts on
    const GfUnit* d_units = gunits.in(c->gf_in.d.p);
    hipLaunchKernelGGL(gf_response_kernel, dim3((unsigned)cdiv(max_w, kGfTile), (unsigned)cdiv(max_h, kGfTile), (unsigned)nu), dim3(kGfTile * kGfTile), 0,
                       c->stream, d_units, K);
    hipLaunchKernelGGL(gf_candidates_kernel, dim3((unsigned)cdiv(max_w, 64), (unsigned)cdiv(max_h, 4), (unsigned)nu), dim3(256), 0, c->stream, d_units, K);
    for (int r = 0; r < kGfRoundLaunches; r++)
        hipLaunchKernelGGL(gf_round_kernel, dim3(kGfRoundBlocks, (unsigned)nu), dim3(256), 0, c->stream, d_units, K);
    hipLaunchKernelGGL(gf_finish_kernel, dim3((unsigned)nu), dim3(kGfFinishThreads), 0, c->stream, d_units, K);
    void* dout = c->gf_out.d.p;
    hipLaunchKernelGGL(gf_output_kernel, dim3(kGfOutBlocks, (unsigned)nj), dim3(256), 0, c->stream, d_units, K, (const GfJob*)gjobs.in(c->gf_in.d.p),
                       (const float2*)have.in(c->gf_in.d.p), cnt.in(dout), oxy.in(dout), oresp.in(dout), ofresh.in(dout));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->gf_out.h.p, c->gf_out.d.p, out.bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->gf_units = nu;
    const void* hout = c->gf_out.h.p;
    const int* h_counts = cnt.in(hout);
    const float2* h_xy = oxy.in(hout);
    const float* h_resp = oresp.in(hout);
    const unsigned char* h_fresh = ofresh.in(hout);
    for (int k = 0; k < nj; k++) {
        const size_t j = (size_t)sel[k];
        std::memcpy(counts + 3 * j, h_counts + 3 * k, sizeof(int) * 3);
        const size_t m = (size_t)std::min(h_counts[3 * k], cap_d);            // what lies past it in the caller's arrays stays as it was
        if (m == 0) continue;
        std::memcpy(xy + 2 * j * capacity, h_xy + (size_t)k * cap_d, sizeof(float2) * m);
        std::memcpy(response + j * capacity, h_resp + (size_t)k * cap_d, sizeof(float) * m);
        std::memcpy(fresh + j * capacity, h_fresh + (size_t)k * cap_d, m);
    }
    return VELO_OK;
}


// velo_detect_features[_batch]: job j runs on the current images of ctxs[job_ctx[j]] (job_ctx null: of ctxs[0])
int gf_detect(velo_ctx** ctxs, int n_ctx, const int32_t* job_ctx, const velo_detect_job* jobs, int32_t n_jobs, const velo_gftt_params* p, int32_t capacity,
              float* xy, float* response, uint8_t* fresh, int32_t* counts) {
    // every argument is checked before any context is touched
    VELO_TRY(fb_check_list(ctxs, n_ctx));
    VELO_TRY(gf_check_params(n_jobs, p, capacity));
    if (n_jobs == 0) return VELO_OK;
    int64_t total = 0;
    VELO_TRY(gf_check_jobs(jobs, n_jobs, capacity, xy, response, fresh, counts, &total));
    VELO_TRY(fb_check_job_ctx(job_ctx, n_jobs, n_ctx));
    VELO_TRY(fb_check_devices(ctxs, n_ctx));
    // the units: the distinct (context, camera) pairs, in the order the jobs name them
    std::vector<GfUnitRef> units;
    std::vector<int> unit_of_job(n_jobs), unit_at((size_t)n_ctx * kLkMaxCams, -1);
    for (int j = 0; j < n_jobs; j++) {
        const int i = fb_ctx_of(job_ctx, j);
        const LkSlot& S = *lk_slot(ctxs[i], false);
        if (!S.valid) return fail(VELO_ERR_STATE, "context %d: no current images: velo_set_images first", i);
        if (jobs[j].cam >= S.n_cams) return fail(VELO_ERR_INVALID, "job %d: camera %d outside the %d that context %d uploaded", j, jobs[j].cam, S.n_cams, i);
        int& u = unit_at[(size_t)i * kLkMaxCams + jobs[j].cam];
        if (u < 0) { u = (int)units.size(); units.push_back(GfUnitRef{i, jobs[j].cam}); }
        unit_of_job[j] = u;
    }
    HIP_TRY(hipSetDevice(ctxs[0]->device));
    std::vector<int> sel;
    for (int u0 = 0; u0 < (int)units.size(); u0 += kGfDetectUnits) {
        const int nu = std::min(kGfDetectUnits, (int)units.size() - u0);
        sel.clear();
        for (int j = 0; j < n_jobs; j++) if (unit_of_job[j] >= u0 && unit_of_job[j] < u0 + nu) sel.push_back(j);
        VELO_TRY(gf_run(ctxs, n_ctx, units, u0, nu, unit_of_job, sel, jobs, p, capacity, xy, response, fresh, counts));
    }
    return VELO_OK;
}

}  // namespace

extern "C" {   // (continued from the previous part)
int velo_default_gftt_params(velo_gftt_params* p) {
    if (!p) return fail(VELO_ERR_INVALID, "null params");
    p->max_corners = 3000; p->block_size = 3; p->quality_level = 0.001; p->min_distance = 12.0;   // kitti.h:7,18,19
    return VELO_OK;
}

int velo_detect_features(velo_ctx* c, const velo_detect_job* jobs, int32_t n_jobs, const velo_gftt_params* p, int32_t capacity, float* xy,
                         float* response, uint8_t* fresh, int32_t* counts) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    return gf_detect(&c, 1, nullptr, jobs, n_jobs, p, capacity, xy, response, fresh, counts);
}

int velo_detect_features_batch(velo_ctx** ctxs, int32_t n_ctx, const int32_t* job_ctx, const velo_detect_job* jobs, int32_t n_jobs,
                               const velo_gftt_params* p, int32_t capacity, float* xy, float* response, uint8_t* fresh, int32_t* counts) {
    if (!job_ctx && n_jobs > 0) return fail(VELO_ERR_INVALID, "null job_ctx");
    return gf_detect(ctxs, n_ctx, job_ctx, jobs, n_jobs, p, capacity, xy, response, fresh, counts);
}

int velo_get_corner_response(velo_ctx* c, int32_t cam, float* out, int64_t capacity_bytes) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    if (!out) return fail(VELO_ERR_INVALID, "null out");
    if (capacity_bytes < 0) return fail(VELO_ERR_INVALID, "negative capacity %lld", (long long)capacity_bytes);
    const LkSlot& S = *lk_slot(c, false);
    if (!S.valid) return fail(VELO_ERR_STATE, "no current images: velo_set_images first");
    if (cam < 0 || cam >= S.n_cams) return fail(VELO_ERR_INVALID, "camera %d of %d", cam, S.n_cams);
    const size_t bytes = sizeof(float) * (size_t)S.w * S.h;
    if ((size_t)capacity_bytes < bytes) return fail(VELO_ERR_INVALID, "capacity %lld bytes < %zu", (long long)capacity_bytes, bytes);
    HIP_TRY(hipSetDevice(c->device));
    // a table of one unit whose only live fields are the image, the map and the header (the response kernel reads nothing else)
    VELO_TRY(c->gf_eig.reserve((size_t)S.w * S.h));
    VELO_TRY(c->gf_hdr.reserve(kGfHdrStride));
    StageLayout in;
    const auto unit = in.add<GfUnit>(1);
    VELO_TRY(c->gf_in.reserve(in.bytes));
    GfUnit& U = *unit.in(c->gf_in.h.p);
    std::memset(&U, 0, sizeof(U));
    U.plane = S.pix.p + (size_t)cam * S.cam_pix + S.pyr.lv[0].off;
    U.eig = c->gf_eig.p;
    U.hdr = c->gf_hdr.p;
    U.w = S.w; U.h = S.h; U.stride = S.pyr.lv[0].stride;
    GfParams K;
    std::memset(&K, 0, sizeof(K));
    K.scale2 = gf_scale2();
    HIP_TRY(hipMemcpyAsync(c->gf_in.d.p, c->gf_in.h.p, in.bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->gf_hdr.p, 0, sizeof(int) * kGfHdrStride, c->stream));
    c->gf_units = 1;
    hipLaunchKernelGGL(gf_response_kernel, dim3((unsigned)cdiv(S.w, kGfTile), (unsigned)cdiv(S.h, kGfTile), 1), dim3(kGfTile * kGfTile), 0, c->stream,
                       (const GfUnit*)unit.in(c->gf_in.d.p), K);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, c->gf_eig.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VELO_OK;
}

#ifdef VELO_DIAGNOSTICS
// diagnostics build only (not declared in velo_hip.h): the per-unit headers of the last detection launch set that the context led (as
// the only or the first context of the call), kGfHdr ints per unit in `out` (maximum bits, candidates, accepted, corners, selection
// passes, undecided when the single-workgroup loop began), units in the order the call's jobs first named them; returns the units
int velo_diag_detect_counters(velo_ctx* c, int* out, int max_units) {
    if (!c || !out) return fail(VELO_ERR_INVALID, "null argument");
    const int n = std::min(c->gf_units, max_units);
    if (n <= 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpy2DAsync(out, sizeof(int) * kGfHdr, c->gf_hdr.p, sizeof(int) * kGfHdrStride, sizeof(int) * kGfHdr, (size_t)n, hipMemcpyDeviceToHost,
                             c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return n;
}
#endif

}  // extern "C"
