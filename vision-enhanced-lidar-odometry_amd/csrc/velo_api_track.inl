// velo_api_track.inl -- part of the host side of the C-ABI, included by velo_hip.hip (ONE translation unit; the order of the parts is the order of
// definition).  C-ABI: resident camera images (velo_set_images, velo_get_image_level) and pyramidal Lucas-Kanade tracking
// (velo_track_features: trackFeatures, velo.h:28-116); kernels in velo_track_kernels.h.
namespace {

int lk_level_count(int w, int h, int win, int max_level) {      // buildOpticalFlowPyramid's deepest level (tests/lk_ref.py level_count)
    for (int lev = 0; lev <= max_level; lev++) {
        if (lev == max_level) return lev;
        w = (w + 1) / 2; h = (h + 1) / 2;
        if (w <= win || h <= win) return lev;
    }
    return max_level;
}

// the stored pyramid of a w x h image: the levels a 5-wide window would build, at most kLkMaxLevel; cam_pix = elements per camera
void lk_plan(LkPyr* P, int w, int h, long long* cam_pix) {
    std::memset(P, 0, sizeof(*P));
    const int top = lk_level_count(w, h, kLkMinWin, kLkMaxLevel);
    long long off = 0;
    for (int lev = 0; lev <= top; lev++) {
        LkLevel& L = P->lv[lev];
        L.w = w; L.h = h; L.stride = w + 2 * kLkPad; L.off = off;
        off += (long long)L.stride * (h + 2 * kLkPad);
        w = (w + 1) / 2; h = (h + 1) / 2;
    }
    P->n_levels = top + 1;
    *cam_pix = (off + 63) & ~63LL;
}

LkSlot* lk_slot(velo_ctx* c, bool previous) { return &c->lk_slot[previous ? (c->lk_cur ^ 1) : c->lk_cur]; }

// the argument checks of velo_track_features that read no context (shared with velo_track_features_batch)
int lk_check_params(int32_t n_jobs, const velo_lk_params* p) {
    if (n_jobs < 0) return fail(VELO_ERR_INVALID, "negative job count %d", n_jobs);
    if (!p) return fail(VELO_ERR_INVALID, "null params");
    if (p->window < kLkMinWin || p->window > kLkMaxWin || (p->window & 1) == 0)
        return fail(VELO_ERR_INVALID, "window %d; odd, %d..%d", p->window, kLkMinWin, kLkMaxWin);
    if (p->max_level < 0 || p->max_level > kLkMaxLevel) return fail(VELO_ERR_INVALID, "max_level %d; 0..%d", p->max_level, kLkMaxLevel);
    if (p->max_count < 0 || p->max_count > 100) return fail(VELO_ERR_INVALID, "max_count %d; 0..100", p->max_count);
    if (!(p->epsilon >= 0.0 && p->epsilon <= 10.0)) return fail(VELO_ERR_INVALID, "epsilon %g; 0..10", p->epsilon);
    if (!std::isfinite(p->min_eig_threshold) || std::isnan(p->flow_outlier)) return fail(VELO_ERR_INVALID, "min_eig_threshold / flow_outlier not a number");
    return VELO_OK;
}

// n_jobs > 0: the job list and the output arrays; *total = points of the call
int lk_check_jobs(const velo_track_job* jobs, int32_t n_jobs, const float* next_xy, const uint8_t* status, const uint8_t* kept, int64_t* total) {
    if (!jobs) return fail(VELO_ERR_INVALID, "null jobs");
    *total = 0;
    for (int j = 0; j < n_jobs; j++) {
        if (jobs[j].n < 0) return fail(VELO_ERR_INVALID, "job %d: negative point count %d", j, jobs[j].n);
        if (jobs[j].n > 0 && !jobs[j].prev_xy) return fail(VELO_ERR_INVALID, "job %d: null points", j);
        *total += jobs[j].n;
    }
    if (*total > (int64_t)(INT32_MAX / 16)) return fail(VELO_ERR_INVALID, "%lld points in one call; at most %d", (long long)*total, INT32_MAX / 16);
    if (*total > 0 && (!next_xy || !status || !kept)) return fail(VELO_ERR_INVALID, "null next_xy / status / kept");
    return VELO_OK;
}

}  // namespace

extern "C" {   // (continued from the previous part)
int velo_set_images(velo_ctx* c, const uint8_t* const* imgs, int32_t n_cams, int32_t width, int32_t height, int32_t stride) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    if (n_cams < 1 || n_cams > kLkMaxCams) return fail(VELO_ERR_INVALID, "%d cameras; 1..%d", n_cams, kLkMaxCams);
    if (!imgs) return fail(VELO_ERR_INVALID, "null image list");
    for (int k = 0; k < n_cams; k++) if (!imgs[k]) return fail(VELO_ERR_INVALID, "image %d is null", k);
    if (width < 1 || height < 1 || width > 16384 || height > 16384) return fail(VELO_ERR_INVALID, "image size %d x %d; 1..16384 each", width, height);
    if (stride < width) return fail(VELO_ERR_INVALID, "row stride %d < width %d", stride, width);
    HIP_TRY(hipSetDevice(c->device));
    // the pinned staging buffer may still be read by the previous call's upload
    if (c->lk_upload_ev) HIP_TRY(hipEventSynchronize(c->lk_upload_ev));
    else HIP_TRY(hipEventCreateWithFlags(&c->lk_upload_ev, hipEventDisableTiming));
    c->lk_cur ^= 1;                                           // current -> previous: a rotation, no copy
    LkSlot& S = c->lk_slot[c->lk_cur];
    S.valid = false;
    LkPyr P;
    long long cam_pix = 0;
    lk_plan(&P, width, height, &cam_pix);
    const size_t raw_bytes = (size_t)n_cams * width * height;
    VELO_TRY(match_pinned((void**)&c->h_lk_raw, &c->h_lk_raw_cap, raw_bytes));
    VELO_TRY(c->lk_raw.reserve(raw_bytes));
    VELO_TRY(S.pix.reserve((size_t)cam_pix * n_cams));
    VELO_TRY(S.der.reserve((size_t)cam_pix * n_cams));
    for (int k = 0; k < n_cams; k++)
        for (int y = 0; y < height; y++)
            std::memcpy(c->h_lk_raw + ((size_t)k * height + y) * width, imgs[k] + (size_t)y * stride, (size_t)width);
    HIP_TRY(hipMemcpyAsync(c->lk_raw.p, c->h_lk_raw, raw_bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(c->lk_upload_ev, c->stream));
    for (int lev = 0; lev < P.n_levels; lev++) {
        const LkLevel& L = P.lv[lev];
        const dim3 grid((unsigned)cdiv(L.w + 2 * kLkPad, kLkTile), (unsigned)cdiv(L.h + 2 * kLkPad, kLkTile), (unsigned)n_cams);
        hipLaunchKernelGGL(lk_build_kernel, grid, dim3(kLkTile * kLkTile), 0, c->stream, (const unsigned char*)c->lk_raw.p, S.pix.p, S.der.p,
                           P, lev, cam_pix);
    }
    HIP_TRY(hipGetLastError());
    S.pyr = P; S.cam_pix = cam_pix; S.n_cams = n_cams; S.w = width; S.h = height; S.valid = true;
    return VELO_OK;
}

int velo_get_image_level(velo_ctx* c, int32_t cam, int32_t previous, int32_t level, int32_t kind, void* out, int64_t capacity_bytes,
                         int32_t* dims) {
    if (!c || !dims) return fail(VELO_ERR_INVALID, "null ctx / dims");
    if (kind < 0 || kind > 2) return fail(VELO_ERR_INVALID, "kind %d; 0 = image, 1 = dx, 2 = dy", kind);
    const LkSlot& S = *lk_slot(c, previous != 0);
    if (!S.valid) return fail(VELO_ERR_STATE, "no %s images: velo_set_images first", previous ? "previous" : "current");
    if (cam < 0 || cam >= S.n_cams) return fail(VELO_ERR_INVALID, "camera %d of %d", cam, S.n_cams);
    if (level < 0 || level >= S.pyr.n_levels) return fail(VELO_ERR_INVALID, "level %d of %d", level, S.pyr.n_levels);
    const LkLevel& L = S.pyr.lv[level];
    dims[0] = L.w; dims[1] = L.h; dims[2] = kLkPad; dims[3] = S.pyr.n_levels;
    if (!out) return VELO_OK;
    if (capacity_bytes < 0) return fail(VELO_ERR_INVALID, "negative capacity %lld", (long long)capacity_bytes);
    const size_t n = (size_t)L.stride * (L.h + 2 * kLkPad);
    if ((size_t)capacity_bytes < n * (kind == 0 ? 1 : 2)) return fail(VELO_ERR_INVALID, "capacity %lld bytes < %zu", (long long)capacity_bytes, n * (kind == 0 ? 1 : 2));
    HIP_TRY(hipSetDevice(c->device));
    if (kind == 0) {
        HIP_TRY(hipMemcpyAsync(out, S.pix.p + (size_t)cam * S.cam_pix + L.off, n, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        return VELO_OK;
    }
    std::vector<int> tmp(n);
    HIP_TRY(hipMemcpyAsync(tmp.data(), S.der.p + (size_t)cam * S.cam_pix + L.off, n * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    int16_t* o = (int16_t*)out;
    for (size_t i = 0; i < n; i++) o[i] = (int16_t)(kind == 1 ? (tmp[i] & 0xFFFF) : (tmp[i] >> 16));
    return VELO_OK;
}

int velo_track_features(velo_ctx* c, const velo_track_job* jobs, int32_t n_jobs, const velo_lk_params* p, float* next_xy, uint8_t* status,
                        uint8_t* kept) {
    // every argument is checked before the context is touched
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    VELO_TRY(lk_check_params(n_jobs, p));
    if (n_jobs == 0) return VELO_OK;
    int64_t total = 0;
    VELO_TRY(lk_check_jobs(jobs, n_jobs, next_xy, status, kept, &total));
    const LkSlot& Sp = *lk_slot(c, true);
    const LkSlot& Sc = *lk_slot(c, false);
    if (!Sp.valid || !Sc.valid) return fail(VELO_ERR_STATE, "tracking needs a previous and a current frame: velo_set_images twice");
    if (Sp.w != Sc.w || Sp.h != Sc.h) return fail(VELO_ERR_INVALID, "previous images are %d x %d, current %d x %d", Sp.w, Sp.h, Sc.w, Sc.h);
    for (int j = 0; j < n_jobs; j++)
        if (jobs[j].prev_cam < 0 || jobs[j].prev_cam >= Sp.n_cams || jobs[j].cam < 0 || jobs[j].cam >= Sc.n_cams)
            return fail(VELO_ERR_INVALID, "job %d: cameras (%d -> %d) outside the uploaded %d / %d", j, jobs[j].prev_cam, jobs[j].cam, Sp.n_cams, Sc.n_cams);
    if (total == 0) return VELO_OK;
    const int n = (int)total;

    HIP_TRY(hipSetDevice(c->device));
    const size_t job_bytes = (sizeof(LkJob) * (size_t)n_jobs + 63) & ~(size_t)63;
    const size_t in_bytes = job_bytes + sizeof(float2) * (size_t)n;
    const size_t out_bytes = sizeof(float2) * (size_t)n + 2 * (size_t)n;
    VELO_TRY(match_pinned((void**)&c->h_lk_in, &c->h_lk_in_cap, in_bytes));
    VELO_TRY(match_pinned((void**)&c->h_lk_out, &c->h_lk_out_cap, out_bytes));
    VELO_TRY(c->lk_in.reserve(in_bytes));
    VELO_TRY(c->lk_out.reserve(out_bytes));
    {
        LkJob* hj = (LkJob*)c->h_lk_in;
        float* hp = (float*)(c->h_lk_in + job_bytes);
        int first = 0;
        for (int j = 0; j < n_jobs; j++) {
            hj[j].prev_cam = jobs[j].prev_cam; hj[j].cam = jobs[j].cam; hj[j].first = first; hj[j].n = jobs[j].n;
            if (jobs[j].n > 0) std::memcpy(hp + 2 * (size_t)first, jobs[j].prev_xy, sizeof(float) * 2 * (size_t)jobs[j].n);
            first += jobs[j].n;
        }
    }
    HIP_TRY(hipMemcpyAsync(c->lk_in.p, c->h_lk_in, in_bytes, hipMemcpyHostToDevice, c->stream));
    LkTrackArgs A;
    std::memset(&A, 0, sizeof(A));
    A.prev_pix = Sp.pix.p; A.prev_der = Sp.der.p; A.cur_pix = Sc.pix.p; A.cam_pix = Sc.cam_pix;
    if (Sp.cam_pix != Sc.cam_pix) return fail(VELO_ERR_STATE, "slot layouts differ");
    A.P = Sc.pyr;
    A.top = std::min(lk_level_count(Sc.w, Sc.h, p->window, p->max_level), Sc.pyr.n_levels - 1);
    A.K.win = p->window; A.K.max_count = p->max_count;
    A.K.min_eig = (float)p->min_eig_threshold;
    A.K.eps2 = p->epsilon * p->epsilon;
    A.K.flow_outlier = p->flow_outlier;
    const LkJob* djobs = (const LkJob*)c->lk_in.p;
    const float2* dpts = (const float2*)(c->lk_in.p + job_bytes);
    float2* oxy = (float2*)c->lk_out.p;
    unsigned char* ost = c->lk_out.p + sizeof(float2) * (size_t)n;
    unsigned char* okp = ost + n;
    unsigned long long* diag = nullptr;
#ifdef VELO_DIAGNOSTICS
    VELO_TRY(c->lk_diag.reserve(2 * kLkLevels));
    if (!c->lk_diag_init) { HIP_TRY(hipMemsetAsync(c->lk_diag.p, 0, sizeof(unsigned long long) * 2 * kLkLevels, c->stream)); c->lk_diag_init = true; }
    diag = c->lk_diag.p;
#endif
    const dim3 grid((unsigned)cdiv(n, kLkThreads / 64));
    const int npl = cdiv(p->window * p->window, 64);
    if (npl <= 4)
        hipLaunchKernelGGL(lk_track_kernel_4, grid, dim3(kLkThreads), 0, c->stream, djobs, n_jobs, dpts, n, A, oxy, ost, okp, diag);
    else if (npl <= 8)
        hipLaunchKernelGGL(lk_track_kernel_8, grid, dim3(kLkThreads), 0, c->stream, djobs, n_jobs, dpts, n, A, oxy, ost, okp, diag);
    else
        hipLaunchKernelGGL(lk_track_kernel_16, grid, dim3(kLkThreads), 0, c->stream, djobs, n_jobs, dpts, n, A, oxy, ost, okp, diag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->h_lk_out, c->lk_out.p, out_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::memcpy(next_xy, c->h_lk_out, sizeof(float2) * (size_t)n);
    std::memcpy(status, c->h_lk_out + sizeof(float2) * (size_t)n, (size_t)n);
    std::memcpy(kept, c->h_lk_out + sizeof(float2) * (size_t)n + n, (size_t)n);
    return VELO_OK;
}

#ifdef VELO_DIAGNOSTICS
// diagnostics build only (not declared in velo_hip.h): out[level] = iterations taken, out[8 + level] = points that entered the iteration
// loop, summed over every velo_track_features call of the context since the last reset (tools/track_bench.py)
int velo_diag_track_counters(velo_ctx* c, unsigned long long* out, int reset) {
    if (!c || !out) return fail(VELO_ERR_INVALID, "null argument");
    std::memset(out, 0, sizeof(unsigned long long) * 2 * kLkLevels);
    if (!c->lk_diag_init) return VELO_OK;
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(hipMemcpyAsync(out, c->lk_diag.p, sizeof(unsigned long long) * 2 * kLkLevels, hipMemcpyDeviceToHost, c->stream));
    if (reset) HIP_TRY(hipMemsetAsync(c->lk_diag.p, 0, sizeof(unsigned long long) * 2 * kLkLevels, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return VELO_OK;
}
#endif

}  // extern "C"
