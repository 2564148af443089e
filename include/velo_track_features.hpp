// velo_track_features.hpp -- header-only C++ adaptor: the reference's feature-tracking functions (velo.h:10-230) on top of
// velo_set_images / velo_track_features (include/velo_hip.h).  C++11.
//
//   FeatureTracker<Matrix3> t(ctx, K, Kinv)      K[cam] / Kinv[cam]: cam_intrinsic / cam_intrinsic_inv (kitti.h), e.g. Eigen::Matrix3f
//   t.setImages(imgs)                            every camera's image of the frame: the current ones become the previous ones (one upload)
//   t.trackFeatures(keypoints, keypoints_p, keypoint_ids, descriptors, img1, img2, cam1, cam2, frame1, frame2)
//                                                velo.h:28-116 with the reference's parameter list; img1 must be the previous image of
//                                                cam1 and img2 the current image of cam2 as handed to setImages (the same data pointer)
//   t.trackFeaturesFrame(keypoints, keypoints_p, keypoint_ids, descriptors, frame)
//                                                main.cpp:222-235: every (cam, prev_cam) pair from frame - 1 into frame, in the reference's
//                                                order (cam outer, prev_cam inner), as ONE call
//   FeatureTracker::setImagesBatch(trackers, imgs) / FeatureTracker::trackFeaturesFrameBatch(trackers, keypoints, keypoints_p,
//   keypoint_ids, descriptors, frames)           several sequences (one tracker and one context each, lists indexed by sequence) in ONE
//                                                library call each (velo_set_images_batch / velo_track_features_batch); per sequence
//                                                exactly what setImages / trackFeaturesFrame do
//   t.consolidateFeatures(keypoints, keypoints_p, keypoint_ids, descriptors, cam)
//                                                velo.h:179-230, host code in the reference's float arithmetic (geomedian: utility.h:105-131)
//   pixel2canonical / canonical2pixel / geomedian velo.h:10-26, utility.h:105-131
//
// Templates, so that it compiles against OpenCV + Eigen or against stand-ins (tests/cpp/track_standin.hpp).  Requirements:
//   Point:   .x, .y (float), Point(float, float)                                        cv::Point2f
//   Matrix3: m(i, j) -> float                                                            Eigen::Matrix3f
//   Image:   .rows, .cols, .data (8-bit, rows `step` bytes apart), (size_t)img.step      cv::Mat (CV_8UC1)
//   Mat:     .rows, .cols, .type(), .row(i), .clone(), .push_back(const Mat&), Mat(rows, cols, type)   cv::Mat of descriptors
// Like the reference, trackFeatures APPENDS to keypoints[cam2][frame2] etc.  The matrix-vector products are (m0 x + m1 y) + m2 with
// every step rounded to float (compile the caller without FMA contraction to reproduce the reference bit for bit).  Errors: a failed
// call throws std::runtime_error with velo_last_error().
#ifndef VELO_TRACK_FEATURES_HPP_
#define VELO_TRACK_FEATURES_HPP_

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <vector>

#include "velo_hip.h"

namespace velo_hip {

// calcOpticalFlowPyrLK's arguments in trackFeatures (kitti.h:5-6,17; velo.h:60-67; OpenCV's default minimum eigenvalue 1e-4)
inline velo_lk_params default_lk_params() {
    velo_lk_params p;
    p.window = 21; p.max_level = 4; p.max_count = 30; p.reserved = 0;
    p.epsilon = 0.01; p.min_eig_threshold = 1e-4; p.flow_outlier = 20000.0;
    return p;
}

template <typename Point, typename Matrix3>
Point mat3_project(const Point& pp, const Matrix3& M) {          // M * (x, y, 1), then (p0 / p2, p1 / p2), all in float
    float p[3];
    for (int i = 0; i < 3; i++) {
        const float a = (float)M(i, 0) * pp.x;
        const float b = (float)M(i, 1) * pp.y;
        const float ab = a + b;
        p[i] = ab + (float)M(i, 2) * 1.0f;
    }
    return Point(p[0] / p[2], p[1] / p[2]);
}
template <typename Point, typename Matrix3>
Point pixel2canonical(const Point& pp, const Matrix3& Kinv) { return mat3_project(pp, Kinv); }   // velo.h:10-17
template <typename Point, typename Matrix3>
Point canonical2pixel(const Point& pp, const Matrix3& K) { return mat3_project(pp, K); }         // velo.h:19-26

template <typename Point>
inline double point_norm(const Point& p) { return std::sqrt((double)p.x * p.x + (double)p.y * p.y); }   // cv::norm(Point2f)

// util::geomedian (utility.h:105-131): Weiszfeld, 20 iterations, eps 1e-6
template <typename Point>
Point geomedian(const std::vector<Point>& P) {
    const float eps = 1e-6f;
    const int m = (int)P.size();
    float yx = 0.f, yy = 0.f;
    for (int i = 0; i < m; i++) { yx = yx + P[i].x; yy = yy + P[i].y; }
    yx = yx / (float)m; yy = yy / (float)m;
    for (int iter = 0; iter < 20; iter++) {
        float ax = 0.f, ay = 0.f, d = 0.f;
        for (int i = 0; i < m; i++) {
            const float no = (float)point_norm(Point(P[i].x - yx, P[i].y - yy));
            if (no < eps) return Point(yx, yy);
            const float nn = (float)(1.0 / no);
            const float px = P[i].x * nn, py = P[i].y * nn;
            ax = ax + px; ay = ay + py;
            d = d + nn;
        }
        const float qx = ax / d, qy = ay / d;
        if (point_norm(Point(qx - yx, qy - yy)) < eps) return Point(qx, qy);
        yx = qx; yy = qy;
    }
    return Point(yx, yy);
}

template <typename Matrix3>
class FeatureTracker {
public:
    FeatureTracker(velo_ctx* ctx, const std::vector<Matrix3>& K, const std::vector<Matrix3>& Kinv,
                   const velo_lk_params& p = default_lk_params())
        : ctx_(ctx), K_(K), Kinv_(Kinv), p_(p) {}

    const velo_lk_params& params() const { return p_; }
    void set_params(const velo_lk_params& p) { p_ = p; }

    // the frame's images, one per camera (8-bit, one size): current -> previous, these -> current
    template <typename Image>
    void setImages(const std::vector<Image>& imgs) {
        const std::vector<const uint8_t*> planes = planes_of(imgs);
        check(velo_set_images(ctx_, planes.data(), (int32_t)planes.size(), (int32_t)imgs[0].cols, (int32_t)imgs[0].rows,
                              (int32_t)(size_t)imgs[0].step), "velo_set_images");
        prev_ = cur_;
        cur_ = planes;
    }

    // setImages of several trackers (one per sequence, distinct contexts on one device) in ONE library call (velo_set_images_batch):
    // imgs[i] are tracker i's images; the sequences may have different image sizes, the number of cameras is the same for all
    template <typename Image>
    static void setImagesBatch(const std::vector<FeatureTracker*>& trackers, const std::vector<std::vector<Image> >& imgs) {
        if (trackers.empty() || trackers.size() != imgs.size()) throw std::runtime_error("setImagesBatch: one image list per tracker");
        std::vector<velo_ctx*> ctxs;
        std::vector<std::vector<const uint8_t*> > planes;
        std::vector<const uint8_t*> all;
        std::vector<int32_t> sizes;
        for (size_t i = 0; i < trackers.size(); i++) {
            planes.push_back(planes_of(imgs[i]));
            if (planes[i].size() != planes[0].size()) throw std::runtime_error("setImagesBatch: every tracker must bring the same number of cameras");
            ctxs.push_back(trackers[i]->ctx_);
            all.insert(all.end(), planes[i].begin(), planes[i].end());
            sizes.push_back((int32_t)imgs[i][0].cols); sizes.push_back((int32_t)imgs[i][0].rows); sizes.push_back((int32_t)(size_t)imgs[i][0].step);
        }
        check(velo_set_images_batch(ctxs.data(), (int32_t)ctxs.size(), all.data(), (int32_t)planes[0].size(), sizes.data()), "velo_set_images_batch");
        for (size_t i = 0; i < trackers.size(); i++) { trackers[i]->prev_ = trackers[i]->cur_; trackers[i]->cur_ = planes[i]; }
    }

    // velo.h:28-116
    template <typename Point, typename Mat, typename Image>
    void trackFeatures(std::vector<std::vector<std::vector<Point> > >& keypoints, std::vector<std::vector<std::vector<Point> > >& keypoints_p,
                       std::vector<std::vector<std::vector<int> > >& keypoint_ids, std::vector<std::vector<Mat> >& descriptors,
                       const Image& img1, const Image& img2, const int cam1, const int cam2, const int frame1, const int frame2) {
        if (cam1 < 0 || cam1 >= (int)prev_.size() || (const uint8_t*)img1.data != prev_[cam1])
            throw std::runtime_error("trackFeatures: img1 is not the previous image of cam1 handed to setImages");
        if (cam2 < 0 || cam2 >= (int)cur_.size() || (const uint8_t*)img2.data != cur_[cam2])
            throw std::runtime_error("trackFeatures: img2 is not the current image of cam2 handed to setImages");
        std::vector<Job> jobs(1, Job(cam1, cam2, frame1, frame2));
        run(keypoints, keypoints_p, keypoint_ids, descriptors, jobs);
    }

    // main.cpp:222-235: trackFeatures(..., img_prevs[prev_cam], imgs[cam], prev_cam, cam, frame - 1, frame) for every pair, one call
    template <typename Point, typename Mat>
    void trackFeaturesFrame(std::vector<std::vector<std::vector<Point> > >& keypoints, std::vector<std::vector<std::vector<Point> > >& keypoints_p,
                            std::vector<std::vector<std::vector<int> > >& keypoint_ids, std::vector<std::vector<Mat> >& descriptors,
                            const int frame) {
        std::vector<Job> jobs;
        for (int cam = 0; cam < (int)cur_.size(); cam++)
            for (int prev_cam = 0; prev_cam < (int)prev_.size(); prev_cam++) jobs.push_back(Job(prev_cam, cam, frame - 1, frame));
        run(keypoints, keypoints_p, keypoint_ids, descriptors, jobs);
    }

    // trackFeaturesFrame of several trackers in ONE library call (velo_track_features_batch): element i of every list is what tracker
    // i's trackFeaturesFrame takes; per tracker the containers receive exactly what its own trackFeaturesFrame appends.  The trackers
    // must share one set of velo_lk_params (the call has one).
    template <typename Point, typename Mat>
    static void trackFeaturesFrameBatch(const std::vector<FeatureTracker*>& trackers,
                                        const std::vector<std::vector<std::vector<std::vector<Point> > >*>& keypoints,
                                        const std::vector<std::vector<std::vector<std::vector<Point> > >*>& keypoints_p,
                                        const std::vector<std::vector<std::vector<std::vector<int> > >*>& keypoint_ids,
                                        const std::vector<std::vector<std::vector<Mat> >*>& descriptors, const std::vector<int>& frames) {
        const size_t n = trackers.size();
        if (n == 0 || keypoints.size() != n || keypoints_p.size() != n || keypoint_ids.size() != n || descriptors.size() != n || frames.size() != n)
            throw std::runtime_error("trackFeaturesFrameBatch: one entry per tracker in every list");
        std::vector<velo_ctx*> ctxs;
        std::vector<Job> jobs;
        std::vector<int32_t> job_ctx;
        for (size_t i = 0; i < n; i++) {
            const FeatureTracker& t = *trackers[i];
            if (std::memcmp(&t.p_, &trackers[0]->p_, sizeof(velo_lk_params)) != 0)
                throw std::runtime_error("trackFeaturesFrameBatch: the trackers of one call must share their velo_lk_params");
            ctxs.push_back(t.ctx_);
            for (int cam = 0; cam < (int)t.cur_.size(); cam++)
                for (int prev_cam = 0; prev_cam < (int)t.prev_.size(); prev_cam++) {
                    jobs.push_back(Job(prev_cam, cam, frames[i] - 1, frames[i]));
                    job_ctx.push_back((int32_t)i);
                }
        }
        std::vector<velo_track_job> cj(jobs.size());
        std::vector<size_t> first(jobs.size() + 1, 0);
        for (size_t j = 0; j < jobs.size(); j++) first[j + 1] = first[j] + keypoints_p[job_ctx[j]]->at(jobs[j].cam1).at(jobs[j].frame1).size();
        std::vector<float> xy(2 * first.back() + 2);
        for (size_t j = 0; j < jobs.size(); j++) fill_job(&cj[j], &xy[2 * first[j]], (*keypoints_p[job_ctx[j]])[jobs[j].cam1][jobs[j].frame1], jobs[j]);
        std::vector<float> next(2 * first.back() + 2);
        std::vector<uint8_t> status(first.back() + 1), kept(first.back() + 1);
        check(velo_track_features_batch(ctxs.data(), (int32_t)n, job_ctx.data(), cj.data(), (int32_t)cj.size(), &trackers[0]->p_, next.data(),
                                        status.data(), kept.data()), "velo_track_features_batch");
        for (size_t j = 0; j < jobs.size(); j++) {
            const size_t i = (size_t)job_ctx[j];
            trackers[i]->append_job(*keypoints[i], *keypoints_p[i], *keypoint_ids[i], *descriptors[i], jobs[j], (size_t)cj[j].n, &next[2 * first[j]],
                                    &kept[first[j]]);
        }
    }

    // velo.h:179-230 (host code): entries merged per id, ids ascending (std::map); n > 2: geomedian, n == 2: the pair mean; the pixel
    // position from canonical2pixel; the descriptor of an id is that of its first occurrence
    template <typename Point, typename Mat>
    void consolidateFeatures(std::vector<Point>& keypoints, std::vector<Point>& keypoints_p, std::vector<int>& keypoint_ids, Mat& descriptors,
                             const int cam) const {
        const Matrix3& K = K_.at(cam);
        std::map<int, std::vector<int> > keypoints_map;
        for (int i = 0; i < (int)keypoint_ids.size(); i++) keypoints_map[keypoint_ids[i]].push_back(i);
        std::vector<Point> tmp_keypoints, tmp_keypoints_p;
        std::vector<int> tmp_ids;
        Mat tmp_descriptors(0, descriptors.cols, descriptors.type());
        for (typename std::map<int, std::vector<int> >::const_iterator it = keypoints_map.begin(); it != keypoints_map.end(); ++it) {
            const std::vector<int>& idx = it->second;
            const int n = (int)idx.size();
            Point gm = keypoints[idx[0]];
            if (n > 2) {
                std::vector<Point> pts;
                for (int i = 0; i < n; i++) pts.push_back(keypoints[idx[i]]);
                gm = geomedian(pts);
            } else if (n == 2) {
                const float sx = keypoints[idx[0]].x + keypoints[idx[1]].x, sy = keypoints[idx[0]].y + keypoints[idx[1]].y;
                gm = Point(sx / 2, sy / 2);
            }
            tmp_ids.push_back(it->first);
            tmp_keypoints.push_back(gm);
            tmp_keypoints_p.push_back(canonical2pixel(gm, K));
            tmp_descriptors.push_back(descriptors.row(idx[0]).clone());
        }
        keypoints = tmp_keypoints;
        keypoints_p = tmp_keypoints_p;
        keypoint_ids = tmp_ids;
        descriptors = tmp_descriptors;
    }

private:
    struct Job {
        int cam1, cam2, frame1, frame2;
        Job(int a, int b, int c, int d) : cam1(a), cam2(b), frame1(c), frame2(d) {}
    };
    static void check(int s, const char* what) {
        if (s != VELO_OK) throw std::runtime_error(std::string(what) + ": " + velo_last_error());
    }

    template <typename Point, typename Mat>
    void run(std::vector<std::vector<std::vector<Point> > >& keypoints, std::vector<std::vector<std::vector<Point> > >& keypoints_p,
             std::vector<std::vector<std::vector<int> > >& keypoint_ids, std::vector<std::vector<Mat> >& descriptors, const std::vector<Job>& jobs) {
        std::vector<velo_track_job> cj(jobs.size());
        std::vector<size_t> first(jobs.size() + 1, 0);
        for (size_t j = 0; j < jobs.size(); j++) first[j + 1] = first[j] + keypoints_p.at(jobs[j].cam1).at(jobs[j].frame1).size();
        std::vector<float> xy(2 * first.back() + 2);
        for (size_t j = 0; j < jobs.size(); j++) fill_job(&cj[j], &xy[2 * first[j]], keypoints_p[jobs[j].cam1][jobs[j].frame1], jobs[j]);
        std::vector<float> next(2 * first.back() + 2);
        std::vector<uint8_t> status(first.back() + 1), kept(first.back() + 1);
        check(velo_track_features(ctx_, cj.data(), (int32_t)cj.size(), &p_, next.data(), status.data(), kept.data()), "velo_track_features");
        for (size_t j = 0; j < jobs.size(); j++)                       // in job order
            append_job(keypoints, keypoints_p, keypoint_ids, descriptors, jobs[j], (size_t)cj[j].n, &next[2 * first[j]], &kept[first[j]]);
    }

    template <typename Image>
    static std::vector<const uint8_t*> planes_of(const std::vector<Image>& imgs) {
        if (imgs.empty()) throw std::runtime_error("setImages: no image");
        std::vector<const uint8_t*> planes;
        for (size_t k = 0; k < imgs.size(); k++) {
            if (imgs[k].rows != imgs[0].rows || imgs[k].cols != imgs[0].cols || (size_t)imgs[k].step != (size_t)imgs[0].step)
                throw std::runtime_error("setImages: every camera's image must have one size and row step");
            planes.push_back((const uint8_t*)imgs[k].data);
        }
        return planes;
    }

    // one velo_track_job: the points of (cam1, frame1), copied to xy
    template <typename Point>
    static void fill_job(velo_track_job* cj, float* xy, const std::vector<Point>& p1, const Job& J) {
        for (size_t i = 0; i < p1.size(); i++) { xy[2 * i] = p1[i].x; xy[2 * i + 1] = p1[i].y; }
        cj->prev_cam = J.cam1;
        cj->cam = J.cam2;
        cj->prev_xy = p1.empty() ? NULL : xy;
        cj->n = (int32_t)p1.size();
    }

    // velo.h:107-114 for one job: next [n][2] and kept [n] as the library returned them
    template <typename Point, typename Mat>
    void append_job(std::vector<std::vector<std::vector<Point> > >& keypoints, std::vector<std::vector<std::vector<Point> > >& keypoints_p,
                    std::vector<std::vector<std::vector<int> > >& keypoint_ids, std::vector<std::vector<Mat> >& descriptors, const Job& J,
                    size_t n, const float* next, const uint8_t* kept) const {
        const Matrix3& Kinv2 = Kinv_.at(J.cam2);
        for (size_t i = 0; i < n; i++) {
            if (!kept[i]) continue;
            const Point p2(next[2 * i], next[2 * i + 1]);
            keypoints_p[J.cam2][J.frame2].push_back(p2);
            keypoints[J.cam2][J.frame2].push_back(pixel2canonical(p2, Kinv2));
            keypoint_ids[J.cam2][J.frame2].push_back(keypoint_ids[J.cam1][J.frame1][i]);
            descriptors[J.cam2][J.frame2].push_back(descriptors[J.cam1][J.frame1].row((int)i).clone());
        }
    }

    velo_ctx* ctx_;
    std::vector<Matrix3> K_, Kinv_;
    velo_lk_params p_;
    std::vector<const uint8_t*> prev_, cur_;   // the images of the last two setImages calls (trackFeatures checks its arguments)
};

}  // namespace velo_hip

#endif  // VELO_TRACK_FEATURES_HPP_
