// velo_landmarks.hpp -- header-only C++11 adaptor of the resident landmark store (velo_landmarks_* in velo_hip.h) over the
// reference's containers: the bookkeeping of main.cpp:614-679 and getLandmarksAtFrame (velo.h:1132-1160, caller main.cpp:376-386).
//
//     velo_hip::LandmarkStore store(ctx, num_cams, &cam_trans[0][0]);
//     per frame:  store.setPose(frame, ceres_poses_vec[frame]);
//                 store.observeFrame(frame, keypoints, keypoint_ids, has_depth, kp_with_depth);      // main.cpp:622-645
//                 store.triangulateFrame(frame, landmarks, keypoint_added);                           // main.cpp:647-679
//     before frameToFrame:  store.landmarksAtFrame(pose_inverse, frame - dframe, landmarks_at_frame);  // main.cpp:376-386
//     every ba_every frames: store.bundleAdjust(window, n_fixed, ceres_poses_vec, landmarks);          // main.cpp:673-725
//
// Templated over the container types (cv::Point2f, pcl::PointCloud<pcl::PointXYZ>::Ptr, Eigen::Matrix4d or stand-ins): a keypoint
// needs .x / .y, a cloud pointer ->points (a vector of points with .x / .y / .z) and a matrix operator()(row, col).
#ifndef VELO_LANDMARKS_HPP_
#define VELO_LANDMARKS_HPP_
#include <map>
#include <vector>

#include "velo_hip.h"

namespace velo_hip {

class LandmarkStore {
public:
    LandmarkStore(velo_ctx* ctx, int num_cams, const float* cam_trans, int log_capacity = 0) : ctx_(ctx), num_cams_(num_cams) {
        status_ = velo_landmarks_reset(ctx, num_cams, cam_trans, log_capacity);
    }
    int status() const { return status_; }

    int setPose(int frame, const double* pose6) { return status_ = velo_landmarks_set_pose(ctx_, frame, pose6); }

    // keypoints[cam][frame][i], keypoint_ids[cam][frame][i], has_depth[cam][frame][i], kp_with_depth[cam][frame]->points[j]
    template <class Keypoints, class Ids, class HasDepth, class Clouds>
    int observeFrame(int frame, const Keypoints& keypoints, const Ids& keypoint_ids, const HasDepth& has_depth, const Clouds& kp_with_depth) {
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
            if (kp_with_depth[cam][frame]) {
                m = kp_with_depth[cam][frame]->points.size();
                cloud.resize(3 * m);
                for (size_t j = 0; j < m; j++) {
                    cloud[3 * j] = kp_with_depth[cam][frame]->points[j].x;
                    cloud[3 * j + 1] = kp_with_depth[cam][frame]->points[j].y;
                    cloud[3 * j + 2] = kp_with_depth[cam][frame]->points[j].z;
                }
            }
            status_ = velo_landmarks_observe(ctx_, frame, cam, n ? &ids[0] : 0, n ? &xy[0] : 0, n ? &hd[0] : 0, m ? &cloud[0] : 0, (int32_t)m, (int32_t)n);
            if (status_ != VELO_OK) return status_;
        }
        return status_;
    }

    // main.cpp:647-679: landmarks->points[id] and keypoint_added[id] of every id triangulated in this frame (both grown as needed)
    template <class CloudPtr>
    int triangulateFrame(int frame, CloudPtr& landmarks, std::vector<bool>& keypoint_added, std::vector<int>* ids_out = 0,
                         std::vector<velo_tri_result>* results_out = 0) {
        int32_t info[8], n_solve = 0;
        if ((status_ = velo_landmarks_info(ctx_, info)) != VELO_OK) return status_;
        if ((status_ = velo_landmarks_frame_count(ctx_, frame, 0, &n_solve)) != VELO_OK) return status_;
        const int32_t cap = n_solve > 0 ? n_solve : 1;         // what this frame will solve, not the id space
        std::vector<int32_t> ids(cap);
        std::vector<float> pts(3 * (size_t)cap);
        std::vector<velo_tri_result> res(cap);
        int32_t n = 0;
        if ((status_ = velo_landmarks_triangulate(ctx_, frame, &ids[0], &pts[0], &res[0], cap, &n)) != VELO_OK) return status_;
        if (landmarks->points.size() < (size_t)info[0]) landmarks->points.resize((size_t)info[0]);
        if (keypoint_added.size() < (size_t)info[0]) keypoint_added.resize((size_t)info[0], false);
        for (int32_t k = 0; k < n; k++) {
            landmarks->points[ids[k]].x = pts[3 * k];
            landmarks->points[ids[k]].y = pts[3 * k + 1];
            landmarks->points[ids[k]].z = pts[3 * k + 2];
            keypoint_added[ids[k]] = true;
        }
        if (ids_out) ids_out->assign(ids.begin(), ids.begin() + n);
        if (results_out) results_out->assign(res.begin(), res.begin() + n);
        return status_;
    }

    // getLandmarksAtFrame with the INVERSE of the frame's pose handed in (pose.inverse() stays the caller's: DESIGN.md 2)
    template <class Matrix4, class Point>
    int landmarksAtFrame(const Matrix4& pose_inverse, int frame, std::map<int, Point>& landmarks_at_frame) {
        double M[16];
        for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) M[4 * r + c] = pose_inverse(r, c);
        int32_t n = 0;
        if ((status_ = velo_landmarks_at_frame(ctx_, frame, M, 0, 0, 0, &n)) != VELO_OK) return status_;
        std::vector<int32_t> ids(n > 0 ? n : 1);
        std::vector<float> xyz(3 * (size_t)(n > 0 ? n : 1));
        if ((status_ = velo_landmarks_at_frame(ctx_, frame, M, &ids[0], &xyz[0], n, &n)) != VELO_OK) return status_;
        for (int32_t k = 0; k < n; k++) {
            Point p;
            p.x = xyz[3 * k]; p.y = xyz[3 * k + 1]; p.z = xyz[3 * k + 2];
            landmarks_at_frame[ids[k]] = p;
        }
        return status_;
    }

    // The BUNDLE_ADJUST step (main.cpp:673-725) over the window `frames` (ascending; the first n_fixed stay constant): refines
    // ceres_poses_vec[frame][0..5] of the free frames and landmarks->points[id] of the landmarks that took part, in the store and in
    // the containers.  ceres_poses_vec[frame] needs operator[] over 6 doubles (double[6], std::vector<double>, ...).
    template <class Poses, class CloudPtr>
    int bundleAdjust(const std::vector<int>& frames, int n_fixed, Poses& ceres_poses_vec, CloudPtr& landmarks, velo_ba_summary* summary = 0,
                     double weight_3d = 1.0) {
        const size_t n = frames.size();
        std::vector<int32_t> fr(frames.begin(), frames.end());
        std::vector<double> poses(6 * (n ? n : 1));
        velo_ba_params params;
        if ((status_ = velo_default_ba_params(&params)) != VELO_OK) return status_;
        params.weight_3d = weight_3d;
        if ((status_ = velo_landmarks_adjust(ctx_, n ? &fr[0] : 0, (int32_t)n, n_fixed, &params, &poses[0], summary)) != VELO_OK) return status_;
        for (size_t i = (size_t)n_fixed; i < n; i++)
            for (int j = 0; j < 6; j++) ceres_poses_vec[frames[i]][j] = poses[6 * i + j];
        int32_t info[8];
        if ((status_ = velo_landmarks_info(ctx_, info)) != VELO_OK) return status_;
        const size_t n_ids = (size_t)info[0];
        if (n_ids == 0) return status_;
        std::vector<int32_t> ids(n_ids);
        std::vector<float> xyz(3 * n_ids);
        std::vector<uint8_t> added(n_ids);
        for (size_t id = 0; id < n_ids; id++) ids[id] = (int32_t)id;
        if ((status_ = velo_landmarks_get(ctx_, &ids[0], (int32_t)n_ids, &xyz[0], &added[0], 0)) != VELO_OK) return status_;
        if (landmarks->points.size() < n_ids) landmarks->points.resize(n_ids);
        for (size_t id = 0; id < n_ids; id++) {
            if (!added[id]) continue;
            landmarks->points[id].x = xyz[3 * id]; landmarks->points[id].y = xyz[3 * id + 1]; landmarks->points[id].z = xyz[3 * id + 2];
        }
        return status_;
    }

private:
    velo_ctx* ctx_;
    int num_cams_;
    int status_;
};

}  // namespace velo_hip
#endif  // VELO_LANDMARKS_HPP_
