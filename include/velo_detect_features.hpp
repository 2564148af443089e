// velo_detect_features.hpp -- header-only C++ adaptor: the reference's detectFeatures (velo.h:118-177) on top of velo_detect_features
// (include/velo_hip.h).  C++11.
//
//   CornerDetector<Matrix3> d(ctx, Kinv)         Kinv[cam]: cam_intrinsic_inv (kitti.h), e.g. Eigen::Matrix3f; parameters: the reference's
//                                                GFTTDetector(3000, 0.001, 12) unless given
//   d.detectFeatures<KeyPoint>(keypoints, keypoints_p, keypoint_ids, descriptors, extractor, img, id_counter, cam, frame)
//                                                velo.h:118-177 with the reference's parameter list; the `detector` argument is replaced by
//                                                the context (detection runs on the CURRENT image of `cam` as uploaded by velo_set_images /
//                                                FeatureTracker::setImages: img must be that image, it is only handed to the extractor)
//   d.detectFeaturesFrame<KeyPoint>(keypoints, keypoints_p, keypoint_ids, descriptors, extractor, imgs, id_counter, frame)
//                                                main.cpp:543-557: every camera of the frame, detection as ONE library call, the
//                                                extraction and the appends camera by camera in the reference's order
//   CornerDetector::detectFeaturesFrameBatch<KeyPoint>(detectors, keypoints, keypoints_p, keypoint_ids, descriptors, extractors, imgs,
//   id_counters, frames)                         several sequences (one detector and one context each, lists indexed by sequence, the
//                                                containers and id counters by pointer) with detection as ONE library call
//                                                (velo_detect_features_batch); per sequence exactly what detectFeaturesFrame does
//
// The descriptor extractor stays the caller's object (cv::Ptr<cv::DescriptorExtractor>, or anything with
// compute(img, std::vector<KeyPoint>&, Mat&) reachable through ->).  As in the reference, "compute MUTATES cvKP": the extractor may
// delete keypoints; the loop runs over what is left and row kp_i of the descriptors belongs to the kp_i-th remaining keypoint.  The
// fresh flag of a remaining keypoint is the library's, found again by its pixel position; a keypoint the extractor moved is tested on
// the host with the same rule.  Detected corners are never added to the occupancy test (velo.h:132-137 fills it before the loop).
// Requirements:
//   Point:    .x, .y (float), Point(float, float)                                        cv::Point2f
//   KeyPoint: KeyPoint(Point, float size), .pt                                            cv::KeyPoint
//   Matrix3:  m(i, j) -> float                                                            Eigen::Matrix3f
//   Mat:      .row(i), .clone(), .push_back(const Mat&)                                   cv::Mat of descriptors
// Errors: a failed call throws std::runtime_error with velo_last_error().
#ifndef VELO_DETECT_FEATURES_HPP_
#define VELO_DETECT_FEATURES_HPP_

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "velo_hip.h"

namespace velo_hip {

inline velo_gftt_params default_gftt_params() {
    velo_gftt_params p;
    if (velo_default_gftt_params(&p) != VELO_OK) throw std::runtime_error(std::string("velo_default_gftt_params: ") + velo_last_error());
    return p;
}

template <typename Point, typename Matrix3>
Point detect_pixel2canonical(const Point& pp, const Matrix3& Kinv) {   // velo.h:10-17; (m0 x + m1 y) + m2, every step rounded to float
    float p[3];
    for (int i = 0; i < 3; i++) {
        const float a = (float)Kinv(i, 0) * pp.x;
        const float b = (float)Kinv(i, 1) * pp.y;
        const float ab = a + b;
        p[i] = ab + (float)Kinv(i, 2) * 1.0f;
    }
    return Point(p[0] / p[2], p[1] / p[2]);
}

template <typename Matrix3>
class CornerDetector {
public:
    CornerDetector(velo_ctx* ctx, const std::vector<Matrix3>& Kinv, const velo_gftt_params& p = default_gftt_params())
        : ctx_(ctx), Kinv_(Kinv), p_(p) {}

    const velo_gftt_params& params() const { return p_; }
    void set_params(const velo_gftt_params& p) { p_ = p; }

    // velo.h:118-177
    template <typename KeyPoint, typename Point, typename Mat, typename ExtractorPtr, typename Image>
    void detectFeatures(std::vector<std::vector<Point> >& keypoints, std::vector<std::vector<Point> >& keypoints_p,
                        std::vector<std::vector<int> >& keypoint_ids, std::vector<Mat>& descriptors, const ExtractorPtr& extractor,
                        const Image& img, int& id_counter, const int cam, const int frame) {
        std::vector<Detected> det;
        std::vector<const std::vector<Point>*> existing(1, &keypoints_p.at(frame));
        std::vector<int> cams(1, cam);
        run(cams, existing, det);
        append<KeyPoint>(det[0], keypoints, keypoints_p, keypoint_ids, descriptors, extractor, img, id_counter, cam, frame);
    }

    // main.cpp:543-557 for every camera: containers indexed [cam][frame]
    template <typename KeyPoint, typename Point, typename Mat, typename ExtractorPtr, typename Image>
    void detectFeaturesFrame(std::vector<std::vector<std::vector<Point> > >& keypoints, std::vector<std::vector<std::vector<Point> > >& keypoints_p,
                             std::vector<std::vector<std::vector<int> > >& keypoint_ids, std::vector<std::vector<Mat> >& descriptors,
                             const ExtractorPtr& extractor, const std::vector<Image>& imgs, int& id_counter, const int frame) {
        std::vector<Detected> det;
        std::vector<const std::vector<Point>*> existing;
        std::vector<int> cams;
        for (int cam = 0; cam < (int)imgs.size(); cam++) { cams.push_back(cam); existing.push_back(&keypoints_p.at(cam).at(frame)); }
        run(cams, existing, det);
        for (int cam = 0; cam < (int)imgs.size(); cam++)
            append<KeyPoint>(det[cam], keypoints[cam], keypoints_p[cam], keypoint_ids[cam], descriptors[cam], extractor, imgs[cam], id_counter,
                             cam, frame);
    }

    // detectFeaturesFrame of several detectors (one per sequence, distinct contexts on one device) in ONE library call
    // (velo_detect_features_batch): element i of every list is what detector i's detectFeaturesFrame takes (extractors[i] and
    // id_counters[i] stay sequence i's own; the extractors run on the host afterwards, sequence by sequence).  Per sequence the
    // containers receive exactly what its own detectFeaturesFrame appends.  The detectors must share one set of velo_gftt_params.
    template <typename KeyPoint, typename Point, typename Mat, typename ExtractorPtr, typename Image>
    static void detectFeaturesFrameBatch(const std::vector<CornerDetector*>& detectors,
                                         const std::vector<std::vector<std::vector<std::vector<Point> > >*>& keypoints,
                                         const std::vector<std::vector<std::vector<std::vector<Point> > >*>& keypoints_p,
                                         const std::vector<std::vector<std::vector<std::vector<int> > >*>& keypoint_ids,
                                         const std::vector<std::vector<std::vector<Mat> >*>& descriptors, const std::vector<ExtractorPtr>& extractors,
                                         const std::vector<std::vector<Image> >& imgs, const std::vector<int*>& id_counters,
                                         const std::vector<int>& frames) {
        const size_t n = detectors.size();
        if (n == 0 || keypoints.size() != n || keypoints_p.size() != n || keypoint_ids.size() != n || descriptors.size() != n ||
            extractors.size() != n || imgs.size() != n || id_counters.size() != n || frames.size() != n)
            throw std::runtime_error("detectFeaturesFrameBatch: one entry per detector in every list");
        std::vector<velo_ctx*> ctxs;
        std::vector<Detected> det;
        std::vector<velo_detect_job> jobs;
        std::vector<int32_t> job_ctx;
        for (size_t i = 0; i < n; i++) {
            if (std::memcmp(&detectors[i]->p_, &detectors[0]->p_, sizeof(velo_gftt_params)) != 0)
                throw std::runtime_error("detectFeaturesFrameBatch: the detectors of one call must share their velo_gftt_params");
            ctxs.push_back(detectors[i]->ctx_);
            std::vector<const std::vector<Point>*> existing;
            std::vector<int> cams;
            for (int cam = 0; cam < (int)imgs[i].size(); cam++) { cams.push_back(cam); existing.push_back(&keypoints_p[i]->at(cam).at(frames[i])); }
            detectors[i]->prepare(cams, existing, det);
            job_ctx.insert(job_ctx.end(), cams.size(), (int32_t)i);
        }
        jobs.resize(det.size());
        for (size_t j = 0; j < det.size(); j++) det[j].job(&jobs[j]);      // after the last push_back: det's buffers no longer move
        detectors[0]->collect(det, jobs, ctxs, &job_ctx);
        size_t j = 0;
        for (size_t i = 0; i < n; i++)
            for (int cam = 0; cam < (int)imgs[i].size(); cam++, j++)
                detectors[i]->template append<KeyPoint>(det[j], (*keypoints[i])[cam], (*keypoints_p[i])[cam], (*keypoint_ids[i])[cam], (*descriptors[i])[cam],
                                                        extractors[i], imgs[i][cam], *id_counters[i], cam, frames[i]);
    }

private:
    struct Detected {
        std::vector<float> xy;
        std::vector<uint8_t> fresh;
        std::vector<float> existing;       // the frame's points when detection ran (the occupancy of velo.h:132-137)
        int width, height, cam;
        void job(velo_detect_job* j) const {
            j->cam = cam;
            j->n_existing = (int32_t)((existing.size() - 2) / 2);
            j->existing_xy = j->n_existing ? existing.data() : NULL;
        }
    };
    static void check(int s, const char* what) {
        if (s != VELO_OK) throw std::runtime_error(std::string(what) + ": " + velo_last_error());
    }

    template <typename Point>
    void run(const std::vector<int>& cams, const std::vector<const std::vector<Point>*>& existing, std::vector<Detected>& det) {
        det.clear();
        prepare(cams, existing, det);
        std::vector<velo_detect_job> jobs(det.size());
        for (size_t j = 0; j < det.size(); j++) det[j].job(&jobs[j]);
        collect(det, jobs, std::vector<velo_ctx*>(1, ctx_), NULL);
    }

    // appends one Detected per camera to det: the image size of this detector's context and the frame's existing points
    template <typename Point>
    void prepare(const std::vector<int>& cams, const std::vector<const std::vector<Point>*>& existing, std::vector<Detected>& det) const {
        int32_t dims[4] = {0, 0, 0, 0};
        check(velo_get_image_level(ctx_, 0, 0, 0, 0, NULL, 0, dims), "velo_get_image_level");
        for (size_t j = 0; j < cams.size(); j++) {
            const std::vector<Point>& e = *existing[j];
            Detected d;
            d.width = dims[0]; d.height = dims[1]; d.cam = cams[j];
            d.existing.resize(2 * e.size() + 2);
            for (size_t i = 0; i < e.size(); i++) { d.existing[2 * i] = e[i].x; d.existing[2 * i + 1] = e[i].y; }
            det.push_back(d);
        }
    }

    // the library call (job_ctx == NULL: this detector's context alone; else the batch entry over ctxs) and its results into det
    void collect(std::vector<Detected>& det, const std::vector<velo_detect_job>& jobs, const std::vector<velo_ctx*>& ctxs,
                 const std::vector<int32_t>* job_ctx) const {
        const size_t n = jobs.size();
        size_t cap = p_.max_corners > 0 ? (size_t)p_.max_corners : 4096;
        std::vector<float> xy, resp;
        std::vector<uint8_t> fresh;
        std::vector<int32_t> counts(3 * n);
        std::vector<velo_ctx*> cs(ctxs);
        for (;;) {
            xy.assign(2 * n * cap, 0.f); resp.assign(n * cap, 0.f); fresh.assign(n * cap, 0);
            if (job_ctx)
                check(velo_detect_features_batch(cs.data(), (int32_t)cs.size(), job_ctx->data(), jobs.data(), (int32_t)n, &p_, (int32_t)cap, xy.data(),
                                                 resp.data(), fresh.data(), counts.data()), "velo_detect_features_batch");
            else
                check(velo_detect_features(ctx_, jobs.data(), (int32_t)n, &p_, (int32_t)cap, xy.data(), resp.data(), fresh.data(), counts.data()),
                      "velo_detect_features");
            size_t need = 0;
            for (size_t j = 0; j < n; j++) if ((size_t)counts[3 * j] > need) need = (size_t)counts[3 * j];
            if (need <= cap) break;
            cap = need;                        // no cap on the corners and more of them than assumed: once more, sized right
        }
        for (size_t j = 0; j < n; j++) {
            const size_t m = (size_t)counts[3 * j];
            det[j].xy.assign(xy.begin() + 2 * j * cap, xy.begin() + 2 * (j * cap + m));
            det[j].fresh.assign(fresh.begin() + j * cap, fresh.begin() + j * cap + m);
        }
    }

    // the rule of velo.h:141-161 for one point, on the host (a keypoint the extractor moved)
    bool host_fresh(const Detected& d, float x, float y) const {
        const float md2 = (float)(p_.min_distance * p_.min_distance);
        const float fw = (float)d.width, fh = (float)d.height;
        for (size_t i = 0; i + 1 < d.existing.size() - 1; i += 2) {
            const float ex = d.existing[i], ey = d.existing[i + 1];
            if (!(ex >= 0.f && ey >= 0.f && ex < fw && ey < fh)) continue;
            const float dx = ex - x, dy = ey - y;
            const float d2 = dx * dx + dy * dy;
            if ((double)d2 < (double)md2) return false;
        }
        return true;
    }

    template <typename KeyPoint, typename Point, typename Mat, typename ExtractorPtr, typename Image>
    void append(const Detected& d, std::vector<std::vector<Point> >& keypoints, std::vector<std::vector<Point> >& keypoints_p,
                std::vector<std::vector<int> >& keypoint_ids, std::vector<Mat>& descriptors, const ExtractorPtr& extractor, const Image& img,
                int& id_counter, const int cam, const int frame) {
        const Matrix3& Kinv = Kinv_.at(cam);
        std::vector<KeyPoint> cvKP;
        std::map<std::pair<float, float>, uint8_t> flag;
        for (size_t i = 0; i < d.fresh.size(); i++) {
            cvKP.push_back(KeyPoint(Point(d.xy[2 * i], d.xy[2 * i + 1]), (float)p_.block_size));
            flag[std::make_pair(d.xy[2 * i], d.xy[2 * i + 1])] = d.fresh[i];
        }
        Mat tmp_descriptors;
        // remember! compute MUTATES cvKP
        extractor->compute(img, cvKP, tmp_descriptors);
        for (int kp_i = 0; kp_i < (int)cvKP.size(); kp_i++) {
            const Point pt = cvKP[kp_i].pt;
            std::map<std::pair<float, float>, uint8_t>::const_iterator it = flag.find(std::make_pair(pt.x, pt.y));
            const bool fresh = it != flag.end() ? it->second != 0 : host_fresh(d, pt.x, pt.y);
            if (!fresh) continue;
            keypoints_p.at(frame).push_back(pt);
            keypoints.at(frame).push_back(detect_pixel2canonical(pt, Kinv));
            descriptors.at(frame).push_back(tmp_descriptors.row(kp_i).clone());
            keypoint_ids.at(frame).push_back(id_counter++);
        }
    }

    velo_ctx* ctx_;
    std::vector<Matrix3> Kinv_;
    velo_gftt_params p_;
};

}  // namespace velo_hip

#endif  // VELO_DETECT_FEATURES_HPP_
