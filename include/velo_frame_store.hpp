// velo_frame_store.hpp -- header-only C++11 adaptor of the resident keypoint frames (velo_frames_*, velo_build_matches in velo_hip.h)
// over the reference's containers: what main.cpp:366-405 does between tracking and frameToFrame, with the visual matches assembled
// on the device.
//
//     velo_hip::FrameStore frames(ctx.get(), num_cams, &cam_trans[0][0]);
//     per frame, once its keypoints, ids and depth are final for a registration (again when they change):
//                 frames.putFrame(keypoints, keypoint_ids, has_depth, keypoints_with_depth, frame);
//     or, instead of projectLidarToCamera + featureDepthAssociation per camera (main.cpp:254-265) and the putFrame / putDescriptors /
//     LandmarkStore::observeFrame that would follow them, with has_depth and keypoints_with_depth made and kept on the device:
//                 frames.putFrameWithDepth(frame, keypoints, keypoint_ids, &descriptors, &bounds[0][0], depth_assoc_thresh, observe);
//     instead of matchUsingId + getLandmarksAtFrame + frameToFrame (main.cpp:366-405):
//                 dpose = velo_hip::frameToFrameResident<Eigen::Matrix4d>(ctx, frames, frame, frame - dframe, &pose_inverse,
//                             scans_M, scans_S, kd_trees, transform, matches, good_matches, residual_type, enable_icp);
//     directly after the dframe == 1 registration, instead of removeSlightlyLessTerribleFeatures (main.cpp:504-514):
//                 frames.pruneFrame(ctx, keypoints, keypoints_p, kp_with_depth, keypoint_ids, descriptors, has_depth, frame);
//     the resident frame and the caller's containers are then what the reference's function leaves, and the frame serves the further
//     diagonal edges, its loop-closure edges and the next frame's edges as it is; good_matches keeps the old indices.  The result of
//     a filter that stays on the host (removeTerribleFeatures) goes in as an index list:
//                 frames.keepFrame(cam, frame, indices, keypoints, keypoints_p, kp_with_depth, keypoint_ids, descriptors, has_depth);
//     frames.dropFrame(frame) when a frame leaves the window.
//     the loop-closure edge (main.cpp:351-365, ba == 1): once a frame's FREAK descriptors are final,
//                 frames.putDescriptors(descriptors, frame);
//     and instead of matchFeatures + getLandmarksAtFrame + frameToFrame for a candidate frame - k:
//                 dpose = velo_hip::frameToFrameLoop<Eigen::Matrix4d>(ctx, frames, frame, frame - k, &pose_inverse, match_thresh,
//                             scans_M, scans_S, kd_trees, transform, matches, good_matches, residual_type, enable_icp);
//     `matches` is matchFeatures' result, for the min_matches gates of main.cpp:366-371.
//
// Templated over the container types like the other adaptors (cv::Point2f, pcl::PointCloud<pcl::PointXYZ>::Ptr, Eigen::Matrix4d or
// stand-ins): a keypoint needs .x / .y, a cloud pointer ->points (a vector of points with .x / .y / .z), a matrix operator()(row, col),
// a descriptor matrix .rows, .cols (64) and .ptr<unsigned char>(row), as cv::Mat has them; pruneFrame / keepFrame also use its
// resize(rows) and the cloud pointer's element_type, push_back and default constructor.
#ifndef VELO_FRAME_STORE_HPP_
#define VELO_FRAME_STORE_HPP_
#include <cstring>
#include <utility>
#include <vector>

#include "velo_frame_to_frame.hpp"

namespace velo_hip {

namespace detail {

// velo.h:302-325 on the containers of one camera of one frame, with the ascending list of kept indices the device wrote in place of
// the std::set: every item moves towards the front, so the containers are compacted in place and cut; the cloud is made anew
template <class Points, class CloudPtr, class IdVec, class Mat, class DepthVec>
void apply_kept(const int32_t* kept, const int m, Points& keypoints, Points& keypoints_p, CloudPtr& kp_with_depth, IdVec& keypoint_ids,
                Mat& descriptors, DepthVec& has_depth) {
    typedef typename CloudPtr::element_type Cloud;
    CloudPtr tmp_kp_with_depth(new Cloud);
    const bool with_p = keypoints_p.size() == keypoints.size(), with_rows = descriptors.rows > 0;
    int jd = 0;
    for (int j = 0; j < m; j++) {
        const size_t i = (size_t)kept[j];
        keypoints[(size_t)j] = keypoints[i];
        if (with_p) keypoints_p[(size_t)j] = keypoints_p[i];
        keypoint_ids[(size_t)j] = keypoint_ids[i];
        if (with_rows && i != (size_t)j)
            std::memmove(descriptors.template ptr<unsigned char>(j), descriptors.template ptr<unsigned char>((int)i), (size_t)descriptors.cols);
        const int d = has_depth[i];
        if (d != -1) {
            tmp_kp_with_depth->push_back(kp_with_depth->points[(size_t)d]);
            has_depth[(size_t)j] = jd++;
        } else {
            has_depth[(size_t)j] = -1;
        }
    }
    keypoints.resize((size_t)m);
    if (with_p) keypoints_p.resize((size_t)m);
    keypoint_ids.resize((size_t)m);
    has_depth.resize((size_t)m);
    if (with_rows) descriptors.resize((size_t)m);
    kp_with_depth = tmp_kp_with_depth;
}

// one frame of one store as velo_frames_put_frame reads it: the staging vectors live as long as the table that points into them
struct PackedFrame {
    std::vector<std::vector<int32_t> > ids;
    std::vector<std::vector<float> > xy;
    std::vector<std::vector<uint8_t> > rows;
    velo_frame_cam cams[8];
    // descriptors: null = no rows; else one 64-byte row per keypoint (a camera without keypoints still holds a row set, an empty one)
    template <class Keypoints, class Ids, class Descriptors>
    int pack(int num_cams, int frame, const Keypoints& keypoints, const Ids& keypoint_ids, const Descriptors* descriptors, const double* bounds) {
        ids.assign((size_t)num_cams, std::vector<int32_t>());
        xy.assign((size_t)num_cams, std::vector<float>());
        rows.assign((size_t)num_cams, std::vector<uint8_t>());
        std::memset(cams, 0, sizeof(cams));
        for (int cam = 0; cam < num_cams; cam++) {
            const size_t n = keypoints[cam][frame].size();
            std::vector<int32_t>& i = ids[(size_t)cam];
            std::vector<float>& k = xy[(size_t)cam];
            i.resize(n + 1);                                            // never empty: &v[0] is an address even for n == 0
            k.resize(2 * n + 2);
            for (size_t j = 0; j < n; j++) {
                i[j] = keypoint_ids[cam][frame][j];
                k[2 * j] = keypoints[cam][frame][j].x;
                k[2 * j + 1] = keypoints[cam][frame][j].y;
            }
            velo_frame_cam& K = cams[cam];
            K.ids = &i[0]; K.keypoints_xy = &k[0]; K.n = (int32_t)n;
            for (int b = 0; b < 4; b++) K.bounds[b] = bounds[4 * cam + b];
            if (!descriptors) continue;
            const int nr = (*descriptors)[cam][frame].rows > 0 ? (*descriptors)[cam][frame].rows : 0;
            if ((size_t)nr != n || (nr > 0 && (*descriptors)[cam][frame].cols != 64)) return VELO_ERR_INVALID;
            std::vector<uint8_t>& r = rows[(size_t)cam];
            r.resize(64 * n + 64);
            for (int j = 0; j < nr; j++) std::memcpy(&r[64 * (size_t)j], (*descriptors)[cam][frame].template ptr<unsigned char>(j), 64);
            K.rows = &r[0];
        }
        return VELO_OK;
    }
};

}  // namespace detail

class FrameStore {
public:
    FrameStore(velo_ctx* ctx, int num_cams, const float* cam_trans, int arena_capacity = 0) : ctx_(ctx), num_cams_(num_cams) {
        status_ = velo_frames_reset(ctx, num_cams, cam_trans, arena_capacity);
    }
    int status() const { return status_; }
    int numCams() const { return num_cams_; }
    velo_ctx* ctx() const { return ctx_; }

    // keypoints[cam][frame][i], keypoint_ids[cam][frame][i], has_depth[cam][frame][i], keypoints_with_depth[cam][frame]->points[j];
    // a frame put before is replaced
    template <class Keypoints, class Ids, class HasDepth, class Clouds>
    int putFrame(const Keypoints& keypoints, const Ids& keypoint_ids, const HasDepth& has_depth, const Clouds& keypoints_with_depth, int frame) {
        for (int cam = 0; cam < num_cams_; cam++) {
            const size_t n = keypoints[cam][frame].size();
            std::vector<int32_t> ids(n), hd(n);
            std::vector<float> xy(2 * n), cloud;
            for (size_t i = 0; i < n; i++) {
                ids[i] = keypoint_ids[cam][frame][i];
                hd[i] = has_depth[cam][frame][i];
                xy[2 * i] = keypoints[cam][frame][i].x;
                xy[2 * i + 1] = keypoints[cam][frame][i].y;
            }
            size_t m = 0;
            if (keypoints_with_depth[cam][frame]) {
                m = keypoints_with_depth[cam][frame]->points.size();
                cloud.resize(3 * m);
                for (size_t j = 0; j < m; j++) {
                    cloud[3 * j] = keypoints_with_depth[cam][frame]->points[j].x;
                    cloud[3 * j + 1] = keypoints_with_depth[cam][frame]->points[j].y;
                    cloud[3 * j + 2] = keypoints_with_depth[cam][frame]->points[j].z;
                }
            }
            status_ = velo_frames_put(ctx_, frame, cam, n ? &ids[0] : 0, n ? &xy[0] : 0, n ? &hd[0] : 0, m ? &cloud[0] : 0, (int32_t)m, (int32_t)n);
            if (status_ != VELO_OK) return status_;
        }
        return status_;
    }

    // descriptors[cam][frame]: one 64-byte row per keypoint of the frame as it was put (rows need not be contiguous: a cv::Mat ROI
    // is gathered); replaces rows put before.  putFrame on the frame drops them: put the descriptors after it.
    template <class Descriptors>
    int putDescriptors(const Descriptors& descriptors, int frame) {
        for (int cam = 0; cam < num_cams_; cam++) {
            const int n = descriptors[cam][frame].rows > 0 ? descriptors[cam][frame].rows : 0;
            if (n > 0 && descriptors[cam][frame].cols != 64) return status_ = VELO_ERR_INVALID;
            std::vector<uint8_t> rows(64 * (size_t)n);
            for (int i = 0; i < n; i++) std::memcpy(&rows[64 * (size_t)i], descriptors[cam][frame].template ptr<unsigned char>(i), 64);
            status_ = velo_frames_put_descriptors(ctx_, frame, cam, n ? &rows[0] : 0, n);
            if (status_ != VELO_OK) return status_;
        }
        return status_;
    }

    // projectLidarToCamera + featureDepthAssociation + putFrame (+ putDescriptors when `descriptors` is not null, + Landmarks::observeFrame
    // with observe) for every camera of `frame` in ONE call, has_depth and keypoints_with_depth made and kept on the device
    // (velo_frames_put_frame): keypoints[cam][frame][i] canonical, keypoint_ids[cam][frame][i], (*descriptors)[cam][frame] one row per
    // keypoint, bounds [num_cams][4] = min_x, max_x, min_y, max_y of every camera.  The scan is the context's source (of_target: its
    // target).  n_with_depth (may be null): the depth points of every camera.  The caller's has_depth / keypoints_with_depth
    // containers are not filled: nothing on the host reads them any more (velo_frames_get does when something must).
    template <class Keypoints, class Ids, class Descriptors>
    int putFrameWithDepth(int frame, const Keypoints& keypoints, const Ids& keypoint_ids, const Descriptors* descriptors, const double* bounds,
                          double thresh, bool observe, bool of_target = false, std::vector<int32_t>* n_with_depth = 0) {
        detail::PackedFrame P;
        if ((status_ = P.pack(num_cams_, frame, keypoints, keypoint_ids, descriptors, bounds)) != VELO_OK) return status_;
        int32_t n_wd[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        status_ = velo_frames_put_frame(ctx_, frame, of_target ? 1 : 0, P.cams, thresh, observe ? VELO_PUT_OBSERVE : 0, n_wd);
        if (status_ == VELO_OK && n_with_depth) n_with_depth->assign(n_wd, n_wd + num_cams_);
        return status_;
    }

    // The same for frames[i] of stores[i] (distinct contexts on one device), i < n, in ONE call (velo_frames_put_frame_batch): the
    // containers, bounds and of_target flags of store i are keypoints[i], keypoint_ids[i], descriptors[i] (the array or an entry may be
    // null), bounds[i], of_target[i] (null: the source everywhere).  Every store's status becomes the call's.
    template <class Keypoints, class Ids, class Descriptors>
    static int putFramesWithDepth(FrameStore* const* stores, int n, const int* frames, const Keypoints* const* keypoints, const Ids* const* keypoint_ids,
                                  const Descriptors* const* descriptors, const double* const* bounds, double thresh, bool observe,
                                  const bool* of_target = 0) {
        if (n < 1 || !stores || !frames || !keypoints || !keypoint_ids || !bounds) return VELO_ERR_INVALID;
        std::vector<detail::PackedFrame> P((size_t)n);
        std::vector<velo_ctx*> ctxs((size_t)n);
        std::vector<int32_t> fr((size_t)n), side((size_t)n, 0), n_wd(8 * (size_t)n, 0);
        std::vector<velo_frame_cam> cams(8 * (size_t)n);
        int status = VELO_OK;
        for (int i = 0; i < n && status == VELO_OK; i++) {
            status = P[(size_t)i].pack(stores[i]->num_cams_, frames[i], *keypoints[i], *keypoint_ids[i], descriptors ? descriptors[i] : 0, bounds[i]);
            std::memcpy(&cams[8 * (size_t)i], P[(size_t)i].cams, sizeof(P[(size_t)i].cams));
            ctxs[(size_t)i] = stores[i]->ctx_;
            fr[(size_t)i] = frames[i];
            side[(size_t)i] = of_target && of_target[i] ? 1 : 0;
        }
        if (status == VELO_OK)
            status = velo_frames_put_frame_batch(&ctxs[0], n, &fr[0], &side[0], &cams[0], thresh, observe ? VELO_PUT_OBSERVE : 0, &n_wd[0]);
        for (int i = 0; i < n; i++) stores[i]->status_ = status;
        return status;
    }

    int dropFrame(int frame) { return status_ = velo_frames_drop(ctx_, frame); }

    // removeSlightlyLessTerribleFeatures(keypoints, ..., frame, good_matches) (velo.h:272-327) with good_matches read on the device:
    // `ctx` holds the visual set frameToFrameResident / frameToFrameLoop built with `frame` as frame1 and the flags of that
    // registration.  The resident frame is pruned on the device (velo_frames_prune); the kept indices come back and cut the caller's
    // containers of every camera to what the reference's function leaves.  Nothing changes when the library refuses the prune.
    template <class Keypoints, class Clouds, class Ids, class Descriptors, class HasDepth>
    int pruneFrame(Context& ctx, Keypoints& keypoints, Keypoints& keypoints_p, Clouds& kp_with_depth, Ids& keypoint_ids, Descriptors& descriptors,
                   HasDepth& has_depth, int frame) {
        if (ctx.get() != ctx_) return status_ = VELO_ERR_INVALID;      // the store lives in another context
        const int32_t cap = frameSize(frame);
        if (status_ != VELO_OK) return status_;
        std::vector<int32_t> n_kept(8, 0), n_wd(8, 0), kept((size_t)(cap > 0 ? cap : 1));
        int32_t total = 0;
        status_ = velo_frames_prune(ctx_, frame, &n_kept[0], &n_wd[0], &kept[0], cap, &total);
        if (status_ != VELO_OK) return status_;
        size_t first = 0;
        for (int cam = 0; cam < num_cams_; cam++) {
            detail::apply_kept(&kept[first], n_kept[(size_t)cam], keypoints[cam][frame], keypoints_p[cam][frame], kp_with_depth[cam][frame],
                               keypoint_ids[cam][frame], descriptors[cam][frame], has_depth[cam][frame]);
            first += (size_t)n_kept[(size_t)cam];
        }
        return status_;
    }

    // The same for ONE camera and an index list (any order, duplicates allowed) made on the host: velo_frames_keep, then the
    // containers of that camera.
    template <class Indices, class Keypoints, class Clouds, class Ids, class Descriptors, class HasDepth>
    int keepFrame(int cam, int frame, const Indices& indices, Keypoints& keypoints, Keypoints& keypoints_p, Clouds& kp_with_depth,
                  Ids& keypoint_ids, Descriptors& descriptors, HasDepth& has_depth) {
        const size_t n = keypoints[cam][frame].size();
        std::vector<int32_t> idx(indices.begin(), indices.end()), kept(n > 0 ? n : 1);
        int32_t n_kept = 0, n_wd = 0;
        status_ = velo_frames_keep(ctx_, frame, cam, idx.empty() ? 0 : &idx[0], (int32_t)idx.size(), &kept[0], (int32_t)n, &n_kept, &n_wd);
        if (status_ != VELO_OK) return status_;
        if ((size_t)n_kept > n) return status_ = VELO_ERR_STATE;       // the containers are not the frame that was put
        detail::apply_kept(&kept[0], n_kept, keypoints[cam][frame], keypoints_p[cam][frame], kp_with_depth[cam][frame], keypoint_ids[cam][frame],
                           descriptors[cam][frame], has_depth[cam][frame]);
        return status_;
    }

    // keypoints of `frame` over all cameras as the library holds them: no match list of a registration against it is longer
    int32_t frameSize(int frame) {
        int32_t n = 0;
        status_ = velo_frames_count(ctx_, frame, 0, &n);
        return status_ == VELO_OK ? n : 0;
    }

private:
    velo_ctx* ctx_;
    int num_cams_;
    int status_;
};

namespace detail {

// what follows the match list in both branches of main.cpp:351-365: the registration on the visual set the build call left, and
// matches / good_matches / residual_type in the reference's containers.  build(M or null, per_cam, pairs, cap, &n) is the build call.
template <typename Mat4, typename CloudPtr, typename ResidualT, typename Build>
Mat4 register_resident(Context& ctx, FrameStore& frames, const int32_t cap, const Mat4* pose2_inverse, const std::vector<CloudPtr>& scans_M,
                       const std::vector<CloudPtr>& scans_S, double transform[6], std::vector<std::vector<std::pair<int, int> > >& matches,
                       std::vector<std::vector<std::pair<int, int> > >& good_matches, std::vector<std::vector<ResidualT> >& residual_type,
                       const bool enable_icp, Build build) {
    velo_params P = ctx.params();
    P.enable_icp = enable_icp ? 1 : 0;                                            // velo.h:806
    ctx.set_params(P);
    if (!scans_S.empty()) ctx.set_target(scans_S);                                // empty: the scan the context already holds
    if (!scans_M.empty()) ctx.set_source(scans_M);

    const int num_cams = frames.numCams();
    double M[16];
    if (pose2_inverse) for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) M[4 * r + c] = (*pose2_inverse)(r, c);
    std::vector<int32_t> per_cam((size_t)num_cams, 0), pairs(2 * (size_t)(cap > 0 ? cap : 1));
    int32_t n = 0;
    build(pose2_inverse ? M : 0, &per_cam[0], &pairs[0], cap, &n);
    matches.assign((size_t)num_cams, std::vector<std::pair<int, int> >());
    for (int cam = 0, k = 0; cam < num_cams; cam++)
        for (int32_t i = 0; i < per_cam[(size_t)cam] && k < cap; i++, k++) matches[(size_t)cam].push_back(std::make_pair((int)pairs[2 * (size_t)k], (int)pairs[2 * (size_t)k + 1]));

    double T[16];
    check(velo_frame_to_frame(ctx.get(), transform, T, 0), "velo_frame_to_frame");

    int32_t ng = 0;
    check(velo_get_good_matches(ctx.get(), 0, 0, &ng), "velo_get_good_matches");
    std::vector<velo_good_match> gm((size_t)ng);
    if (ng > 0) check(velo_get_good_matches(ctx.get(), &gm[0], ng, &ng), "velo_get_good_matches");
    good_matches.resize((size_t)num_cams);
    residual_type.resize((size_t)num_cams);
    for (int cam = 0; cam < num_cams; cam++) { good_matches[(size_t)cam].clear(); residual_type[(size_t)cam].clear(); }
    for (size_t k = 0; k < gm.size(); k++) {
        good_matches[(size_t)gm[k].cam].push_back(std::make_pair(gm[k].point1, gm[k].point2));
        residual_type[(size_t)gm[k].cam].push_back((ResidualT)gm[k].residual_type);
    }
    Mat4 out;
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) out(i, j) = T[i * 4 + j];
    return out;
}

struct BuildById {
    velo_ctx* ctx; int frame1, frame2;
    void operator()(const double* M, int32_t* per_cam, int32_t* pairs, int32_t cap, int32_t* n) const {
        check(velo_build_matches(ctx, frame1, frame2, M, per_cam, pairs, cap, n), "velo_build_matches");
    }
};

struct BuildByDescriptor {
    velo_ctx* ctx; int frame1, frame2; double match_thresh;
    void operator()(const double* M, int32_t* per_cam, int32_t* pairs, int32_t cap, int32_t* n) const {
        check(velo_build_matches_desc(ctx, frame1, frame2, M, match_thresh, per_cam, pairs, cap, n), "velo_build_matches_desc");
    }
};

}  // namespace detail

// frameToFrame (velo.h:598-614) for two frames of `frames`, which lives in `ctx`: the matches (matchUsingId, velo.h:562-590), the
// landmarks of frame2 (getLandmarksAtFrame with the INVERSE pose handed in; null: no landmarks) and the gather of velo.h:627-654 run
// on the device, then the registration as in frameToFrame.  `matches` receives matchUsingId's result for the caller's min_matches
// tests (main.cpp:366-371); good_matches / residual_type as frameToFrame fills them.
template <typename Mat4, typename CloudPtr, typename KdTrees, typename ResidualT>
Mat4 frameToFrameResident(Context& ctx, FrameStore& frames, const int frame1, const int frame2, const Mat4* pose2_inverse,
                          const std::vector<CloudPtr>& scans_M, const std::vector<CloudPtr>& scans_S,
                          const KdTrees& /*kd_trees: superseded by the device grid*/,
                          double transform[6],
                          std::vector<std::vector<std::pair<int, int> > >& matches,
                          std::vector<std::vector<std::pair<int, int> > >& good_matches,
                          std::vector<std::vector<ResidualT> >& residual_type,
                          const bool enable_icp) {
    const detail::BuildById build = {ctx.get(), frame1, frame2};
    return detail::register_resident<Mat4>(ctx, frames, frames.frameSize(frame2), pose2_inverse, scans_M, scans_S, transform, matches,
                                           good_matches, residual_type, enable_icp, build);
}

// The loop-closure edge (main.cpp:351-365 with ba == 1): frameToFrameResident with the matches made by matchFeatures on the two
// frames' resident descriptor rows (query = frame1, train = frame2, velo.h:499-560) instead of matchUsingId.  `matches` receives
// matchFeatures' result.
template <typename Mat4, typename CloudPtr, typename KdTrees, typename ResidualT>
Mat4 frameToFrameLoop(Context& ctx, FrameStore& frames, const int frame1, const int frame2, const Mat4* pose2_inverse, const double match_thresh,
                      const std::vector<CloudPtr>& scans_M, const std::vector<CloudPtr>& scans_S,
                      const KdTrees& /*kd_trees: superseded by the device grid*/,
                      double transform[6],
                      std::vector<std::vector<std::pair<int, int> > >& matches,
                      std::vector<std::vector<std::pair<int, int> > >& good_matches,
                      std::vector<std::vector<ResidualT> >& residual_type,
                      const bool enable_icp) {
    const detail::BuildByDescriptor build = {ctx.get(), frame1, frame2, match_thresh};
    return detail::register_resident<Mat4>(ctx, frames, frames.frameSize(frame1), pose2_inverse, scans_M, scans_S, transform, matches,
                                           good_matches, residual_type, enable_icp, build);
}

}  // namespace velo_hip
#endif  // VELO_FRAME_STORE_HPP_
