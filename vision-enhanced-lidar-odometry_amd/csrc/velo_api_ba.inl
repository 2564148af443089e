// velo_api_ba.inl -- part of the host side of the C-ABI, included by velo_hip.hip (ONE translation unit; the order of the parts is the order of
// definition).  C-ABI: bundle adjustment of a window of frames over the resident landmark store (velo_landmarks_adjust*); the kernels
// and the scheme of one LM iteration are in velo_ba_kernels.h.
//
// The host knows the window and the ids its frames observed; which of them take part is decided on the device (only it knows `added`),
// and the host reads the count once.  From then on it launches the five kernels of an iteration and reads one 64-byte record to learn
// whether to go on.  Every buffer belongs to the store and keeps its size between calls.
struct BaWork {
    DevBuf<int> cand, n_obs, n_3d, sel, hdr;
    DevBuf<velo_tri_obs> obs;
    DevBuf<BaState> st;
    DevBuf<double> xc, pt, lin, blk, scale_p, diag_p, lterm, red, sch;
    DevBuf<unsigned> fmask;
    PinBuf<> h_in, h_out;
    Event in_ev;
};

namespace {

struct BaCall {
    BaArgs A;
    BaWork* W;
    int n_cand, L, n_blocks, n_residuals;
};

int ba_check(velo_ctx* c, const int32_t* frames, int32_t n_frames, int32_t n_fixed, const velo_ba_params* params, const char* who) {
    if (!c) return fail(VELO_ERR_INVALID, "null ctx");
    if (!frames) return fail(VELO_ERR_INVALID, "%s: null frames", who);
    if (n_fixed < 1) return fail(VELO_ERR_INVALID, "%s: %d fixed frames; at least 1 fixes the gauge", who, n_fixed);
    const int64_t n_free = (int64_t)n_frames - n_fixed;
    if (n_free < 1 || n_free > VELO_BA_MAX_FREE) return fail(VELO_ERR_INVALID, "%s: %lld free frames; 1..%d", who, (long long)n_free, VELO_BA_MAX_FREE);
    for (int i = 0; i < n_frames; i++) {
        VELO_TRY(check_frame(frames[i], who));
        if (i > 0 && frames[i] <= frames[i - 1]) return fail(VELO_ERR_INVALID, "%s: frames must be ascending and distinct (%d after %d)", who, frames[i], frames[i - 1]);
    }
    if (params && !(params->weight_3d > 0.0 && std::isfinite(params->weight_3d))) return fail(VELO_ERR_INVALID, "%s: weight_3d must be positive and finite", who);
    VELO_TRY(lm_need_store(c, who));
    const LmStore& S = *c->lm;
    if ((int64_t)n_frames * S.n_cams > kBaMaxObs) return fail(VELO_ERR_INVALID, "%s: %d frames x %d cameras; at most %d observations of a landmark", who, n_frames, S.n_cams, kBaMaxObs);
    for (int i = 0; i < n_frames; i++)
        if ((size_t)frames[i] >= S.pose_set.size() || !S.pose_set[(size_t)frames[i]]) return fail(VELO_ERR_STATE, "%s: frame %d has no pose: velo_landmarks_set_pose", who, frames[i]);
    return VELO_OK;
}

// select, gather, count (one read-back), widen the points, linearise at the stored state and reduce: the system at the start
int ba_begin(velo_ctx* c, const int32_t* frames, int32_t n_frames, int32_t n_fixed, const velo_ba_params* params, BaCall* call) {
    LmStore& S = *c->lm;
    if (!S.ba) S.ba = std::make_shared<BaWork>();
    BaWork& W = *std::static_pointer_cast<BaWork>(S.ba);
    HIP_TRY(hipSetDevice(c->device));
    std::vector<int32_t> cand, ids;
    for (int i = 0; i < n_frames; i++) {
        lm_frame_ids(S, frames[i], &ids);
        cand.insert(cand.end(), ids.begin(), ids.end());
    }
    std::sort(cand.begin(), cand.end());
    cand.erase(std::unique(cand.begin(), cand.end()), cand.end());
    const int nc = (int)cand.size(), n_free = n_frames - n_fixed;
    BaArgs& A = call->A;
    std::memset(&A, 0, sizeof(A));
    call->W = &W; call->n_cand = nc; call->L = 0; call->n_blocks = 0; call->n_residuals = 0;
    A.W.n_frames = n_frames; A.W.n_fixed = n_fixed; A.W.n_free = n_free; A.W.n_cams = S.n_cams;
    for (int i = 0; i < n_frames; i++) A.W.frames[i] = frames[i];
    A.P.lm = lm_params(c->P);
    A.P.loss_a = c->P.loss_thresh_3D2D; A.P.loss_w = c->P.weight_3D2D;      // velo.h:1116-1119
    A.weight_3d = params ? params->weight_3d : 1.0;
    if (nc == 0) return VELO_OK;
    const size_t n_red = (size_t)n_free * kBaRed + kBaScalars;
    VELO_TRY(W.cand.reserve((size_t)nc));
    VELO_TRY(W.n_obs.reserve((size_t)nc));
    VELO_TRY(W.n_3d.reserve((size_t)nc));
    VELO_TRY(W.sel.reserve((size_t)nc));
    VELO_TRY(W.hdr.reserve(4));
    VELO_TRY(W.obs.reserve((size_t)nc * kBaMaxObs));
    VELO_TRY(W.st.reserve(1));
    VELO_TRY(W.xc.reserve((size_t)2 * kBaMaxObs * 6));
    VELO_TRY(W.red.reserve(2 * ((size_t)VELO_BA_MAX_FREE * kBaRed + kBaScalars)));
    VELO_TRY(W.sch.reserve((size_t)(VELO_BA_MAX_FREE * (VELO_BA_MAX_FREE + 1) / 2) * 36 + 6 * VELO_BA_MAX_FREE));
    VELO_TRY(W.in_ev.wait_or_create());
    VELO_TRY(W.h_in.reserve(sizeof(int32_t) * (size_t)nc));
    VELO_TRY(W.h_out.reserve(sizeof(double) * (2 * n_red + 2 * (size_t)kBaMaxObs * 6) + sizeof(BaState) + 64));
    std::memcpy(W.h_in.p, cand.data(), sizeof(int32_t) * (size_t)nc);
    HIP_TRY(hipMemcpyAsync(W.cand.p, W.h_in.p, sizeof(int32_t) * (size_t)nc, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(W.in_ev, c->stream));
    A.frames = S.frames.p; A.cam_t = S.cam_t.p; A.log = S.log.p; A.prev = S.prev.p; A.head = S.head.p; A.pts = S.pts.p; A.added = S.added.p;
    A.cand_ids = W.cand.p; A.n_cand = nc;
    A.obs = W.obs.p; A.n_obs = W.n_obs.p; A.n_3d = W.n_3d.p; A.sel = W.sel.p; A.hdr = W.hdr.p; A.st = W.st.p; A.xc = W.xc.p;
    A.red = W.red.p; A.sch = W.sch.p;
    hipLaunchKernelGGL(ba_gather_kernel, dim3((unsigned)nc), dim3(64), 0, c->stream, A);
    hipLaunchKernelGGL(ba_compact_kernel, dim3(1), dim3(256), 0, c->stream, A, nc);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(W.h_out.p, W.hdr.p, sizeof(int) * 3, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const int* hdr = (const int*)W.h_out.p;
    const int L = hdr[0];
    call->L = L; call->n_blocks = hdr[1]; call->n_residuals = hdr[2];
    if (L <= 0 || L > nc) { call->L = 0; return L == 0 ? VELO_OK : fail(VELO_ERR_HIP, "the selection counted %d of %d landmarks", L, nc); }
    const size_t Lz = (size_t)L;
    VELO_TRY(W.pt.reserve(2 * Lz * 3));
    VELO_TRY(W.lin.reserve(2 * Lz * kBaLin));
    VELO_TRY(W.blk.reserve(2 * Lz * (size_t)n_free * kBaBlk));
    VELO_TRY(W.scale_p.reserve(Lz * 3));
    VELO_TRY(W.diag_p.reserve(Lz * 3));
    VELO_TRY(W.lterm.reserve(Lz * 4));
    VELO_TRY(W.fmask.reserve(Lz));
    A.pt = W.pt.p; A.lin = W.lin.p; A.blk = W.blk.p; A.scale_p = W.scale_p.p; A.diag_p = W.diag_p.p; A.lterm = W.lterm.p; A.fmask = W.fmask.p;
    A.L = L;
    hipLaunchKernelGGL(ba_points_in_kernel, dim3((unsigned)cdiv(L, 256)), dim3(256), 0, c->stream, A);
    hipLaunchKernelGGL(ba_linearize_kernel, dim3((unsigned)L), dim3(64), 0, c->stream, A, 0);
    hipLaunchKernelGGL(ba_reduce_kernel, dim3((unsigned)n_red), dim3(256), 0, c->stream, A, 0);
    HIP_TRY(hipGetLastError());
    return VELO_OK;
}

}  // namespace

extern "C" {   // (continued from the previous part)
int velo_default_ba_params(velo_ba_params* p) {
    if (!p) return fail(VELO_ERR_INVALID, "null params");
    std::memset(p, 0, sizeof(*p));
    p->weight_3d = 1.0;
    return VELO_OK;
}

int velo_landmarks_adjust_system(velo_ctx* c, const int32_t* frames, int32_t n_frames, int32_t n_fixed, const velo_ba_params* params, double* cost,
                                 double* gradient, double* JtJ_pose) {
    VELO_TRY(ba_check(c, frames, n_frames, n_fixed, params, "velo_landmarks_adjust_system"));
    const int n_free = n_frames - n_fixed;
    BaCall call;
    VELO_TRY(ba_begin(c, frames, n_frames, n_fixed, params, &call));
    if (cost) *cost = 0.0;
    if (gradient) std::memset(gradient, 0, sizeof(double) * 6 * (size_t)n_free);
    if (JtJ_pose) std::memset(JtJ_pose, 0, sizeof(double) * 36 * (size_t)n_free);
    if (call.L == 0) return VELO_OK;
    BaWork& W = *call.W;
    const size_t n_red = (size_t)n_free * kBaRed + kBaScalars;
    HIP_TRY(hipMemcpyAsync(W.h_out.p, W.red.p, sizeof(double) * n_red, hipMemcpyDeviceToHost, c->stream));   // the state starts in buffer 0
    HIP_TRY(hipStreamSynchronize(c->stream));
    const double* red = (const double*)W.h_out.p;
    if (cost) *cost = red[n_free * kBaRed];
    for (int k = 0; k < n_free; k++) expand_upper6(red + k * kBaRed, gradient ? gradient + 6 * k : nullptr, JtJ_pose ? JtJ_pose + 36 * k : nullptr);
    return VELO_OK;
}

int velo_landmarks_adjust(velo_ctx* c, const int32_t* frames, int32_t n_frames, int32_t n_fixed, const velo_ba_params* params, double* poses_out,
                          velo_ba_summary* summary) {
    VELO_TRY(ba_check(c, frames, n_frames, n_fixed, params, "velo_landmarks_adjust"));
    const int n_free = n_frames - n_fixed;
    LmStore& S = *c->lm;
    velo_ba_summary sum;
    std::memset(&sum, 0, sizeof(sum));
    sum.termination = VELO_CONVERGENCE;
    sum.evaluations = 1;
    // the poses as they are: what a call that moves nothing returns (TriFrame keeps -omega and the centre)
    std::vector<double> poses((size_t)n_frames * 6);
    for (int i = 0; i < n_frames; i++) {
        const TriFrame& F = S.h_frames.p[frames[i]];
        for (int j = 0; j < 3; j++) { poses[(size_t)i * 6 + j] = -F.w[j]; poses[(size_t)i * 6 + 3 + j] = F.center[j]; }
    }
    BaCall call;
    VELO_TRY(ba_begin(c, frames, n_frames, n_fixed, params, &call));
    sum.n_landmarks = call.L; sum.n_blocks = call.n_blocks; sum.n_residuals = call.n_residuals;
    if (call.L > 0) {
        BaWork& W = *call.W;
        const BaArgs& A = call.A;
        const size_t n_red = (size_t)n_free * kBaRed + kBaScalars;
        const unsigned n_schur = (unsigned)(n_free * (n_free + 1) / 2 + n_free);
        BaRecord* rec = (BaRecord*)W.h_out.p;
        hipLaunchKernelGGL(ba_decide_kernel, dim3(1), dim3(64), 0, c->stream, A, 0);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(rec, W.st.p, sizeof(BaRecord), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        sum.initial_cost = rec->cost;
        while (!rec->done) {
            hipLaunchKernelGGL(ba_schur_kernel, dim3(n_schur), dim3(256), 0, c->stream, A);
            hipLaunchKernelGGL(ba_solve_kernel, dim3(1), dim3(64), 0, c->stream, A);
            hipLaunchKernelGGL(ba_linearize_kernel, dim3((unsigned)call.L), dim3(64), 0, c->stream, A, 1);
            hipLaunchKernelGGL(ba_reduce_kernel, dim3((unsigned)n_red), dim3(256), 0, c->stream, A, 1);
            hipLaunchKernelGGL(ba_decide_kernel, dim3(1), dim3(64), 0, c->stream, A, 1);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(rec, W.st.p, sizeof(BaRecord), hipMemcpyDeviceToHost, c->stream));    // the one record of the iteration
            HIP_TRY(hipStreamSynchronize(c->stream));
            if (sum.n_trace < VELO_BA_MAX_TRACE) {
                velo_ba_iteration& t = sum.trace[sum.n_trace++];
                t.status = rec->status; t.iteration = rec->iteration; t.cost = rec->cost; t.candidate_cost = rec->candidate_cost;
                t.radius = rec->radius; t.model_change = rec->model_change; t.step_norm = rec->step_norm;
            }
        }
        sum.termination = rec->termination; sum.iterations = rec->iteration; sum.evaluations = rec->evaluations;
        // the points back as float, the free poses and the final cost to the host
        unsigned char* tail = W.h_out.p + 64;
        hipLaunchKernelGGL(ba_points_out_kernel, dim3((unsigned)cdiv(call.L, 256)), dim3(256), 0, c->stream, A);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(tail, W.st.p, sizeof(BaState), hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(tail + sizeof(BaState), W.xc.p, sizeof(double) * 2 * (size_t)n_frames * 6, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        const BaState* st = (const BaState*)tail;
        const double* xc = (const double*)(tail + sizeof(BaState)) + (size_t)st->cur * n_frames * 6;
        sum.final_cost = st->tr.cost;
        if (st->tr.n_accepted > 0) {
            for (int i = n_fixed; i < n_frames; i++) {
                for (int j = 0; j < 6; j++) poses[(size_t)i * 6 + j] = xc[(size_t)i * 6 + j];
                VELO_TRY(velo_landmarks_set_pose(c, frames[i], &poses[(size_t)i * 6]));    // the frame table's one host path
            }
        }
    }
    if (poses_out) std::memcpy(poses_out, poses.data(), sizeof(double) * poses.size());
    if (summary) *summary = sum;
    return VELO_OK;
}

}  // extern "C"
