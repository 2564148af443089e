// velo_api_detect.inl -- part of the host side of the C-ABI, included by velo_hip.hip (ONE translation unit; the order of the parts is the order of
// definition).  C-ABI: GFTT corner detection on the current resident images (velo_detect_features: detectFeatures, velo.h:118-177;
// velo_get_corner_response); kernels in velo_detect_kernels.h.
namespace {

// buffers and kernel arguments for `n_units` cameras of the current slot; everything a call zeroes is zeroed here (stream-ordered)
int gf_prepare(velo_ctx* c, const LkSlot& S, const int* cams, int n_units, GfArgs* A) {
    std::memset(A, 0, sizeof(*A));
    const size_t plane = (size_t)S.w * S.h;
    const int sstride = (S.w + 2 * kGfStatePad + 3) & ~3;
    const size_t splane = (size_t)sstride * (S.h + 2 * kGfStatePad);
    size_t keys_cap = 1;
    while (keys_cap < plane) keys_cap <<= 1;
    VELO_TRY(c->gf_eig.reserve(plane * n_units));
    VELO_TRY(c->gf_state.reserve(splane * n_units));
    VELO_TRY(c->gf_cand.reserve(2 * plane * n_units));
    VELO_TRY(c->gf_keys.reserve(keys_cap * n_units));
    VELO_TRY(c->gf_hdr.reserve((size_t)kGfHdr * kGfMaxUnits));
    A->pix = S.pix.p; A->cam_pix = S.cam_pix; A->L0 = S.pyr.lv[0];
    A->w = S.w; A->h = S.h; A->n_units = n_units;
    for (int u = 0; u < n_units; u++) A->cams[u] = cams[u];
    A->eig = c->gf_eig.p;
    A->state = c->gf_state.p; A->sstride = sstride; A->splane = (long long)splane;
    A->cand = c->gf_cand.p; A->und = c->gf_cand.p + plane * n_units;
    A->keys = c->gf_keys.p; A->keys_cap = (long long)keys_cap;
    A->hdr = c->gf_hdr.p;
    const float s = (float)(1.0 / (255.0 * 4.0 * 3.0));       // cornerMinEigenVal: 1 / (255 * 2^(ksize - 1) * blockSize)
    A->K.scale2 = s * s;
    HIP_TRY(hipMemsetAsync(c->gf_hdr.p, 0, sizeof(int) * kGfHdr * kGfMaxUnits, c->stream));
    c->gf_units = n_units;
    return VELO_OK;
}

// the argument checks of velo_detect_features that read no context (shared with velo_detect_features_batch)
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
        if (jobs[j].cam < 0 || jobs[j].cam >= kLkMaxCams) return fail(VELO_ERR_INVALID, "job %d: camera %d; 0..%d", j, jobs[j].cam, kLkMaxCams - 1);
        *total += jobs[j].n_existing;
    }
    if (n_jobs > 4096) return fail(VELO_ERR_INVALID, "%d jobs in one call; at most 4096", n_jobs);
    if (*total > (int64_t)(INT32_MAX / 16)) return fail(VELO_ERR_INVALID, "%lld points in one call; at most %d", (long long)*total, INT32_MAX / 16);
    return VELO_OK;
}

void gf_launch_response(velo_ctx* c, const GfArgs& A) {
    const dim3 grid((unsigned)cdiv(A.w, kGfTile), (unsigned)cdiv(A.h, kGfTile), (unsigned)A.n_units);
    hipLaunchKernelGGL(gf_response_kernel, grid, dim3(kGfTile * kGfTile), 0, c->stream, A);
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
    // every argument is checked before the context is touched
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    VELO_TRY(gf_check_params(n_jobs, p, capacity));
    if (n_jobs == 0) return VELO_OK;
    int64_t total = 0;
    VELO_TRY(gf_check_jobs(jobs, n_jobs, capacity, xy, response, fresh, counts, &total));
    const LkSlot& S = *lk_slot(c, false);
    if (!S.valid) return fail(VELO_ERR_STATE, "no current images: velo_set_images first");
    int cams[kGfMaxUnits], unit_of[kLkMaxCams], n_units = 0;
    for (int k = 0; k < kLkMaxCams; k++) unit_of[k] = -1;
    for (int j = 0; j < n_jobs; j++) {
        if (jobs[j].cam >= S.n_cams) return fail(VELO_ERR_INVALID, "job %d: camera %d outside the uploaded %d", j, jobs[j].cam, S.n_cams);
        if (unit_of[jobs[j].cam] < 0) { unit_of[jobs[j].cam] = n_units; cams[n_units++] = jobs[j].cam; }
    }
    const size_t plane = (size_t)S.w * S.h;
    const int cap_d = (int)std::min<size_t>((size_t)capacity, plane);        // a camera has at most one corner per pixel

    HIP_TRY(hipSetDevice(c->device));
    GfArgs A;
    VELO_TRY(gf_prepare(c, S, cams, n_units, &A));
    A.K.radius = (int)std::ceil(p->min_distance) - 1;
    A.K.max_corners = p->max_corners;
    A.K.capacity = cap_d;
    A.K.quality = p->quality_level;
    A.K.md2 = p->min_distance * p->min_distance;
    A.K.md2f = (float)(p->min_distance * p->min_distance);
    const size_t job_bytes = (sizeof(GfJob) * (size_t)n_jobs + 63) & ~(size_t)63;
    const size_t in_bytes = job_bytes + sizeof(float2) * (size_t)total;
    const size_t cnt_bytes = (sizeof(int) * 3 * (size_t)n_jobs + 63) & ~(size_t)63;
    const size_t n_slots = (size_t)n_jobs * cap_d;
    const size_t out_bytes = cnt_bytes + n_slots * (sizeof(float2) + sizeof(float) + 1);
    VELO_TRY(match_pinned((void**)&c->h_gf_in, &c->h_gf_in_cap, in_bytes));
    VELO_TRY(match_pinned((void**)&c->h_gf_out, &c->h_gf_out_cap, out_bytes));
    VELO_TRY(c->gf_in.reserve(in_bytes));
    VELO_TRY(c->gf_out.reserve(out_bytes));
    {
        GfJob* hj = (GfJob*)c->h_gf_in;
        float* hp = (float*)(c->h_gf_in + job_bytes);
        int first = 0;
        for (int j = 0; j < n_jobs; j++) {
            hj[j].unit = unit_of[jobs[j].cam]; hj[j].first = first; hj[j].n = jobs[j].n_existing; hj[j].pad_ = 0;
            if (jobs[j].n_existing > 0) std::memcpy(hp + 2 * (size_t)first, jobs[j].existing_xy, sizeof(float) * 2 * (size_t)jobs[j].n_existing);
            first += jobs[j].n_existing;
        }
    }
    HIP_TRY(hipMemcpyAsync(c->gf_in.p, c->h_gf_in, in_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemsetAsync(c->gf_state.p, 0, (size_t)A.splane * n_units, c->stream));      // the zero border of the state maps
    HIP_TRY(hipMemsetAsync(c->gf_out.p, 0, cnt_bytes, c->stream));
    gf_launch_response(c, A);
    hipLaunchKernelGGL(gf_candidates_kernel, dim3((unsigned)cdiv(A.w, 64), (unsigned)cdiv(A.h, 4), (unsigned)n_units), dim3(256), 0, c->stream, A);
    for (int r = 0; r < kGfRoundLaunches; r++)
        hipLaunchKernelGGL(gf_round_kernel, dim3(kGfRoundBlocks, (unsigned)n_units), dim3(256), 0, c->stream, A);
    hipLaunchKernelGGL(gf_finish_kernel, dim3((unsigned)n_units), dim3(kGfFinishThreads), 0, c->stream, A);
    int* d_counts = (int*)c->gf_out.p;
    float2* d_xy = (float2*)(c->gf_out.p + cnt_bytes);
    float* d_resp = (float*)(c->gf_out.p + cnt_bytes + n_slots * sizeof(float2));
    unsigned char* d_fresh = c->gf_out.p + cnt_bytes + n_slots * (sizeof(float2) + sizeof(float));
    hipLaunchKernelGGL(gf_output_kernel, dim3(kGfOutBlocks, (unsigned)n_jobs), dim3(256), 0, c->stream, A, (const GfJob*)c->gf_in.p,
                       (const float2*)(c->gf_in.p + job_bytes), d_counts, d_xy, d_resp, d_fresh);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_gf_out, c->gf_out.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int* h_counts = (const int*)c->h_gf_out;
    const unsigned char* h_xy = c->h_gf_out + cnt_bytes;
    const unsigned char* h_resp = h_xy + n_slots * sizeof(float2);
    const unsigned char* h_fresh = h_resp + n_slots * sizeof(float);
    std::memcpy(counts, h_counts, sizeof(int) * 3 * (size_t)n_jobs);
    for (int j = 0; j < n_jobs; j++) {
        const size_t m = (size_t)std::min(h_counts[3 * j], cap_d);            // what lies past it in the caller's arrays stays as it was
        if (m == 0) continue;
        std::memcpy(xy + 2 * (size_t)j * capacity, h_xy + sizeof(float2) * (size_t)j * cap_d, sizeof(float2) * m);
        std::memcpy(response + (size_t)j * capacity, h_resp + sizeof(float) * (size_t)j * cap_d, sizeof(float) * m);
        std::memcpy(fresh + (size_t)j * capacity, h_fresh + (size_t)j * cap_d, m);
    }
    return VELO_OK;
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
    GfArgs A;
    const int cams[1] = {cam};
    VELO_TRY(gf_prepare(c, S, cams, 1, &A));
    gf_launch_response(c, A);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(out, c->gf_eig.p, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VELO_OK;
}

#ifdef VELO_DIAGNOSTICS
// diagnostics build only (not declared in velo_hip.h): the per-unit header of the last velo_detect_features call, kGfHdr ints per unit
// (maximum bits, candidates, accepted, corners, selection passes, undecided when the single-workgroup loop began); returns the units
int velo_diag_detect_counters(velo_ctx* c, int* out, int max_units) {
    if (!c || !out) return fail(VELO_ERR_INVALID, "null argument");
    const int n = std::min(c->gf_units, max_units);
    if (n <= 0) return 0;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(out, c->gf_hdr.p, sizeof(int) * kGfHdr * (size_t)n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return n;
}
#endif

}  // extern "C"
