// velo_api_track.inl -- part of the host side of the C-ABI, included by velo_hip.hip (ONE translation unit; the order of the parts is the order of
// definition).  C-ABI: resident camera images (velo_set_images[_batch], velo_get_image_level) and pyramidal Lucas-Kanade tracking
// (velo_track_features[_batch]: trackFeatures, velo.h:28-116); kernels in velo_track_kernels.h.
//
// Every stage of the visual front end (images and tracking here, detection in velo_api_detect.inl) has ONE implementation, over a list
// of contexts; the single-context entries hand it a list of one.  Who owns what: the FIRST context of a call (ctxs[0]) lends its
// stream and its staging pairs (lk_raw / lk_in / lk_out, gf_*: pinned and device buffer, velo_host_types.inl); every context keeps its
// own image slots, and the kernels write / read them through per-unit tables that ride in the call's one upload, laid out by a
// StageLayout (velo_stage_layout.h).  Mixed image sizes are served by the SAME launches: a table entry carries its unit's size, grids
// are sized for the largest unit.  The checks of the list and the hand-over are velo_host_types.inl's (fb_*).
// Hand-over between the streams: the lending stream first waits for an event recorded on every other named context's stream; the
// synchronous entries (track, detect) end in a synchronisation of the lending stream, after which nothing of the call is in flight;
// the asynchronous one (set_images) records an event on the lending stream that every other context's stream then waits for.  With
// one context there is no other stream: no event is recorded or waited for.
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

// the argument checks of tracking that read no context
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

// index of the level table of a w x h image in `pyrs` (appended when new)
int fb_pyr_index(std::vector<LkPyr>* pyrs, std::vector<long long>* cam_pix, int w, int h) {
    for (size_t k = 0; k < pyrs->size(); k++) if ((*pyrs)[k].lv[0].w == w && (*pyrs)[k].lv[0].h == h) return (int)k;
    LkPyr P;
    long long cp = 0;
    lk_plan(&P, w, h, &cp);
    pyrs->push_back(P);
    cam_pix->push_back(cp);
    return (int)pyrs->size() - 1;
}

// velo_set_images[_batch]: imgs[i * n_cams + k] is camera k of context i, sizes[3 i ..] = {width, height, stride} of context i
int lk_set_images(velo_ctx** ctxs, int n_ctx, const uint8_t* const* imgs, int n_cams, const int32_t* sizes) {
    // every argument is checked before any context is touched
    VELO_TRY(fb_check_list(ctxs, n_ctx));
    if (n_cams < 1 || n_cams > kLkMaxCams) return fail(VELO_ERR_INVALID, "%d cameras; 1..%d", n_cams, kLkMaxCams);
    if (!imgs) return fail(VELO_ERR_INVALID, "null image list");
    if (!sizes) return fail(VELO_ERR_INVALID, "null sizes");
    for (int i = 0; i < n_ctx; i++) {
        for (int k = 0; k < n_cams; k++) if (!imgs[(size_t)i * n_cams + k]) return fail(VELO_ERR_INVALID, "context %d: image %d is null", i, k);
        const int w = sizes[3 * i], h = sizes[3 * i + 1], st = sizes[3 * i + 2];
        if (w < 1 || h < 1 || w > 16384 || h > 16384) return fail(VELO_ERR_INVALID, "context %d: image size %d x %d; 1..16384 each", i, w, h);
        if (st < w) return fail(VELO_ERR_INVALID, "context %d: row stride %d < width %d", i, st, w);
    }
    VELO_TRY(fb_check_devices(ctxs, n_ctx));
    velo_ctx* c = ctxs[0];
    HIP_TRY(hipSetDevice(c->device));
    // the pinned staging buffer may still be read by the previous call's upload
    VELO_TRY(c->lk_upload_ev.wait_or_create());
    std::vector<LkPyr> pyrs;
    std::vector<long long> cam_pix;
    std::vector<int> pyr_of(n_ctx);
    size_t raw_bytes = 0;
    for (int i = 0; i < n_ctx; i++) {
        pyr_of[i] = fb_pyr_index(&pyrs, &cam_pix, sizes[3 * i], sizes[3 * i + 1]);
        raw_bytes += (size_t)n_cams * sizes[3 * i] * sizes[3 * i + 1];
    }
    const int n_units = n_ctx * n_cams;
    StageLayout in;
    const auto units = in.add<LkBuildUnit>((size_t)n_units);
    const auto levels = in.add<LkPyr>(pyrs.size());
    const auto raw = in.add<unsigned char>(raw_bytes);
    VELO_TRY(c->lk_raw.reserve(in.bytes));
    // The slot every context is about to fill is its previous one (current -> previous is a rotation, no copy).  Every allocation comes
    // first and nothing rotates unless everything was allocated: a failure leaves every context's current and previous images as they
    // were, except a previous slot whose buffer had to be replaced.
    for (int i = 0; i < n_ctx; i++) {
        LkSlot& S = ctxs[i]->lk_slot[ctxs[i]->lk_cur ^ 1];
        const size_t need = (size_t)cam_pix[pyr_of[i]] * n_cams;
        if (need > S.pix.cap || need > S.der.cap) S.valid = false;   // growing frees the old buffer: that slot's images are gone either way
        VELO_TRY(S.pix.reserve(need));
        VELO_TRY(S.der.reserve(need));
    }
    for (int i = 0; i < n_ctx; i++) ctxs[i]->lk_slot[ctxs[i]->lk_cur ^ 1].valid = false;
    {
        LkBuildUnit* hu = units.in(c->lk_raw.h.p);
        std::memcpy(levels.in(c->lk_raw.h.p), pyrs.data(), levels.size());
        size_t off = 0;                                       // into the raw images
        for (int i = 0; i < n_ctx; i++) {
            const int w = sizes[3 * i], h = sizes[3 * i + 1], st = sizes[3 * i + 2];
            LkSlot& S = ctxs[i]->lk_slot[ctxs[i]->lk_cur ^ 1];
            for (int k = 0; k < n_cams; k++) {
                LkBuildUnit& U = hu[i * n_cams + k];
                U.raw = raw.in(c->lk_raw.d.p) + off;
                U.pix = S.pix.p + (size_t)k * cam_pix[pyr_of[i]];
                U.der = S.der.p + (size_t)k * cam_pix[pyr_of[i]];
                U.pyr = pyr_of[i]; U.pad_ = 0;
                const uint8_t* src = imgs[(size_t)i * n_cams + k];
                for (int y = 0; y < h; y++) std::memcpy(raw.in(c->lk_raw.h.p) + off + (size_t)y * w, src + (size_t)y * st, (size_t)w);
                off += (size_t)w * h;
            }
        }
    }
    VELO_TRY(fb_gather(ctxs, n_ctx, nullptr));
    HIP_TRY(hipMemcpyAsync(c->lk_raw.d.p, c->lk_raw.h.p, in.bytes, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(c->lk_upload_ev, c->stream));
    int max_levels = 0;
    for (const LkPyr& P : pyrs) max_levels = std::max(max_levels, P.n_levels);
    for (int lev = 0; lev < max_levels; lev++) {
        int mw = 0, mh = 0;                                   // the largest unit that has this level
        for (const LkPyr& P : pyrs) if (lev < P.n_levels) { mw = std::max(mw, P.lv[lev].w); mh = std::max(mh, P.lv[lev].h); }
        const dim3 grid((unsigned)cdiv(mw + 2 * kLkPad, kLkTile), (unsigned)cdiv(mh + 2 * kLkPad, kLkTile), (unsigned)n_units);
        hipLaunchKernelGGL(lk_build_kernel, grid, dim3(kLkTile * kLkTile), 0, c->stream, units.in(c->lk_raw.d.p),
                           levels.in(c->lk_raw.d.p), lev);
    }
    HIP_TRY(hipGetLastError());
    VELO_TRY(fb_release(ctxs, n_ctx));
    for (int i = 0; i < n_ctx; i++) {
        velo_ctx* ci = ctxs[i];
        ci->lk_cur ^= 1;
        LkSlot& S = ci->lk_slot[ci->lk_cur];
        S.pyr = pyrs[pyr_of[i]]; S.cam_pix = cam_pix[pyr_of[i]]; S.n_cams = n_cams; S.w = sizes[3 * i]; S.h = sizes[3 * i + 1]; S.valid = true;
    }
    return VELO_OK;
}

// velo_track_features[_batch]: job j runs on ctxs[job_ctx[j]] (job_ctx null: on ctxs[0])
int lk_track(velo_ctx** ctxs, int n_ctx, const int32_t* job_ctx, const velo_track_job* jobs, int32_t n_jobs, const velo_lk_params* p, float* next_xy,
             uint8_t* status, uint8_t* kept) {
    // every argument is checked before any context is touched
    VELO_TRY(fb_check_list(ctxs, n_ctx));
    VELO_TRY(lk_check_params(n_jobs, p));
    if (n_jobs == 0) return VELO_OK;
    int64_t total = 0;
    VELO_TRY(lk_check_jobs(jobs, n_jobs, next_xy, status, kept, &total));
    VELO_TRY(fb_check_job_ctx(job_ctx, n_jobs, n_ctx));
    VELO_TRY(fb_check_devices(ctxs, n_ctx));
    std::vector<char> used(n_ctx, 0);
    for (int j = 0; j < n_jobs; j++) {
        const int i = fb_ctx_of(job_ctx, j);
        const LkSlot& Sp = *lk_slot(ctxs[i], true);
        const LkSlot& Sc = *lk_slot(ctxs[i], false);
        if (!used[i]) {
            if (!Sp.valid || !Sc.valid) return fail(VELO_ERR_STATE, "context %d: tracking needs a previous and a current frame: velo_set_images twice", i);
            if (Sp.w != Sc.w || Sp.h != Sc.h || Sp.cam_pix != Sc.cam_pix)
                return fail(VELO_ERR_INVALID, "context %d: previous images are %d x %d, current %d x %d", i, Sp.w, Sp.h, Sc.w, Sc.h);
            used[i] = 1;
        }
        if (jobs[j].prev_cam < 0 || jobs[j].prev_cam >= Sp.n_cams || jobs[j].cam < 0 || jobs[j].cam >= Sc.n_cams)
            return fail(VELO_ERR_INVALID, "job %d: cameras (%d -> %d) outside the %d / %d that context %d uploaded", j, jobs[j].prev_cam, jobs[j].cam, Sp.n_cams,
                        Sc.n_cams, i);
    }
    if (total == 0) return VELO_OK;
    const int n = (int)total;
    velo_ctx* c = ctxs[0];
    HIP_TRY(hipSetDevice(c->device));
    std::vector<LkPyr> pyrs;
    std::vector<long long> cam_pix;
    std::vector<int> pyr_of(n_ctx, -1);
    for (int i = 0; i < n_ctx; i++) if (used[i]) pyr_of[i] = fb_pyr_index(&pyrs, &cam_pix, lk_slot(ctxs[i], false)->w, lk_slot(ctxs[i], false)->h);
    StageLayout in, out;
    const auto ljobs = in.add<LkJob>((size_t)n_jobs);
    const auto levels = in.add<LkPyr>(pyrs.size());
    const auto pts = in.add<float2>((size_t)n);
    const auto oxy = out.add<float2>((size_t)n);
    const auto ost = out.add<unsigned char>((size_t)n, 1);      // packed: status and kept start wherever the points end
    const auto okp = out.add<unsigned char>((size_t)n, 1);
    VELO_TRY(c->lk_in.reserve(in.bytes));
    VELO_TRY(c->lk_out.reserve(out.bytes));
    {
        LkJob* hj = ljobs.in(c->lk_in.h.p);
        std::memcpy(levels.in(c->lk_in.h.p), pyrs.data(), levels.size());
        float* hp = (float*)pts.in(c->lk_in.h.p);
        int first = 0;
        for (int j = 0; j < n_jobs; j++) {
            const int i = fb_ctx_of(job_ctx, j);
            const LkSlot& Sp = *lk_slot(ctxs[i], true);
            const LkSlot& Sc = *lk_slot(ctxs[i], false);
            hj[j].first = first; hj[j].n = jobs[j].n;
            hj[j].pyr = pyr_of[i];
            hj[j].top = std::min(lk_level_count(Sc.w, Sc.h, p->window, p->max_level), Sc.pyr.n_levels - 1);
            hj[j].prev_pix = Sp.pix.p + (size_t)jobs[j].prev_cam * Sp.cam_pix;
            hj[j].prev_der = Sp.der.p + (size_t)jobs[j].prev_cam * Sp.cam_pix;
            hj[j].cur_pix = Sc.pix.p + (size_t)jobs[j].cam * Sc.cam_pix;
            if (jobs[j].n > 0) std::memcpy(hp + 2 * (size_t)first, jobs[j].prev_xy, sizeof(float) * 2 * (size_t)jobs[j].n);
            first += jobs[j].n;
        }
    }
    VELO_TRY(fb_gather(ctxs, n_ctx, &used));
    HIP_TRY(hipMemcpyAsync(c->lk_in.d.p, c->lk_in.h.p, in.bytes, hipMemcpyHostToDevice, c->stream));
    LkParams K;
    std::memset(&K, 0, sizeof(K));
    K.win = p->window; K.max_count = p->max_count;
    K.min_eig = (float)p->min_eig_threshold;
    K.eps2 = p->epsilon * p->epsilon;
    K.flow_outlier = p->flow_outlier;
    const void* din = c->lk_in.d.p;
    void* dout = c->lk_out.d.p;
    unsigned long long* diag = nullptr;
#ifdef VELO_DIAGNOSTICS
    VELO_TRY(c->lk_diag.reserve(2 * kLkLevels));
    if (!c->lk_diag_init) { HIP_TRY(hipMemsetAsync(c->lk_diag.p, 0, sizeof(unsigned long long) * 2 * kLkLevels, c->stream)); c->lk_diag_init = true; }
    diag = c->lk_diag.p;
#endif
    const dim3 grid((unsigned)cdiv(n, kLkThreads / 64));
    const int npl = cdiv(p->window * p->window, 64);
    if (npl <= 4)
        hipLaunchKernelGGL(lk_track_kernel_4, grid, dim3(kLkThreads), 0, c->stream, ljobs.in(din), n_jobs, levels.in(din), pts.in(din), n, K, oxy.in(dout), ost.in(dout), okp.in(dout), diag);
    else if (npl <= 8)
        hipLaunchKernelGGL(lk_track_kernel_8, grid, dim3(kLkThreads), 0, c->stream, ljobs.in(din), n_jobs, levels.in(din), pts.in(din), n, K, oxy.in(dout), ost.in(dout), okp.in(dout), diag);
    else
        hipLaunchKernelGGL(lk_track_kernel_16, grid, dim3(kLkThreads), 0, c->stream, ljobs.in(din), n_jobs, levels.in(din), pts.in(din), n, K, oxy.in(dout), ost.in(dout), okp.in(dout), diag);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->lk_out.h.p, c->lk_out.d.p, out.bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const void* hout = c->lk_out.h.p;
    std::memcpy(next_xy, oxy.in(hout), oxy.size());
    std::memcpy(status, ost.in(hout), ost.size());
    std::memcpy(kept, okp.in(hout), okp.size());
    return VELO_OK;
}

}  // namespace

extern "C" {   // (continued from the previous part)
int velo_set_images(velo_ctx* c, const uint8_t* const* imgs, int32_t n_cams, int32_t width, int32_t height, int32_t stride) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    const int32_t sizes[3] = {width, height, stride};
    return lk_set_images(&c, 1, imgs, n_cams, sizes);
}

int velo_set_images_batch(velo_ctx** ctxs, int32_t n_ctx, const uint8_t* const* imgs, int32_t n_cams, const int32_t* sizes) {
    return lk_set_images(ctxs, n_ctx, imgs, n_cams, sizes);
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
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    return lk_track(&c, 1, nullptr, jobs, n_jobs, p, next_xy, status, kept);
}

int velo_track_features_batch(velo_ctx** ctxs, int32_t n_ctx, const int32_t* job_ctx, const velo_track_job* jobs, int32_t n_jobs,
                              const velo_lk_params* p, float* next_xy, uint8_t* status, uint8_t* kept) {
    if (!job_ctx && n_jobs > 0) return fail(VELO_ERR_INVALID, "null job_ctx");
    return lk_track(ctxs, n_ctx, job_ctx, jobs, n_jobs, p, next_xy, status, kept);
}

#ifdef VELO_DIAGNOSTICS
// diagnostics build only (not declared in velo_hip.h): out[level] = iterations taken, out[8 + level] = points that entered the iteration
// loop, summed over every tracking call that the context led (as the only or the first context) since the last reset (tools/track_bench.py)
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
