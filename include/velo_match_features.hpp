// velo_match_features.hpp -- header-only C++ adaptor: the reference's descriptor-matching functions (velo.h:499-590) on top of
// velo_match_descriptors (include/velo_hip.h).  C++11.
//
//   matchFeatures(descriptors, cam1, cam2, frame1, frame2, matches)   velo.h:499-550  (replaces both the USE_CUDA branch, velo.h:517-525,
//                                                                                       and cv::BFMatcher, velo.h:527-531)
//   matchFeatures(descriptors, frame1, frame2, matches)               velo.h:551-560  every camera in ONE call
//   matchUsingId(keypoint_ids, cam1, cam2, frame1, frame2, matches)   velo.h:562-579  plain host code, as in the reference
//   matchUsingId(keypoint_ids, frame1, frame2, matches)               velo.h:580-590
//   matchFeaturesBatch(descriptors, frame, candidate_frames, matches_per_candidate)
//                                 the loop-closure stage (main.cpp:351-364): every camera of every candidate frame in ONE call
//
// It is a template over the descriptor matrix so that it compiles against cv::Mat when OpenCV is present and against a stand-in
// (tests/cpp/mat_standin.hpp) when it is not.  Requirements on Mat, all satisfied by cv::Mat of FREAK descriptors (CV_8U, 64 columns):
//   m.rows, m.cols (64, or any value with rows == 0), m.ptr<unsigned char>(r) -> the 64 bytes of row r.
// A matrix whose rows are not contiguous (a cv::Mat ROI) is gathered into a buffer of the matcher first; a contiguous one is passed
// as it is.  The camera count of the per-frame forms is descriptors.size() / keypoint_ids.size() (the reference's num_cams,
// kitti.h).  Like the reference, every form APPENDS to the vectors it is given.  Errors: a failed call throws std::runtime_error with
// velo_last_error().
#ifndef VELO_MATCH_FEATURES_HPP_
#define VELO_MATCH_FEATURES_HPP_

#include <cstdint>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "velo_hip.h"

namespace velo_hip {

class DescriptorMatcher {
public:
    // ctx: a context of include/velo_hip.h (matching leaves its registration state alone); match_thresh: kitti.h:27
    explicit DescriptorMatcher(velo_ctx* ctx, double match_thresh = 29.0) : ctx_(ctx), match_thresh_(match_thresh) {}

    double match_thresh() const { return match_thresh_; }
    void set_match_thresh(double t) { match_thresh_ = t; }

    // velo.h:499-550
    template <typename Mat>
    void matchFeatures(const std::vector<std::vector<Mat> >& descriptors, const int cam1, const int cam2, const int frame1, const int frame2,
                       std::vector<std::pair<int, int> >& matches) {
        begin();
        add_job(descriptors[cam1][frame1], descriptors[cam2][frame2]);
        std::vector<std::vector<std::pair<int, int> >*> out(1, &matches);
        run(out);
    }

    // velo.h:551-560: matchFeatures(descriptors, cam, cam, frame1, frame2, matches[cam]) for every camera, one call
    template <typename Mat>
    void matchFeatures(const std::vector<std::vector<Mat> >& descriptors, const int frame1, const int frame2,
                       std::vector<std::vector<std::pair<int, int> > >& matches) {
        begin();
        std::vector<std::vector<std::pair<int, int> >*> out;
        for (size_t cam = 0; cam < descriptors.size(); cam++) {
            add_job(descriptors[cam][frame1], descriptors[cam][frame2]);
            out.push_back(&matches.at(cam));
        }
        run(out);
    }

    // the loop-closure candidates of one frame (main.cpp:351-364): matches_per_candidate[c][cam] receives
    // matchFeatures(descriptors, cam, cam, frame, candidate_frames[c], ...), every camera of every candidate in one call; the
    // query matrix of a camera is uploaded once for all candidates
    template <typename Mat>
    void matchFeaturesBatch(const std::vector<std::vector<Mat> >& descriptors, const int frame, const std::vector<int>& candidate_frames,
                            std::vector<std::vector<std::vector<std::pair<int, int> > > >& matches_per_candidate) {
        begin();
        const size_t n_cams = descriptors.size();
        if (matches_per_candidate.size() < candidate_frames.size()) matches_per_candidate.resize(candidate_frames.size());
        std::vector<std::vector<std::pair<int, int> >*> out;
        for (size_t c = 0; c < candidate_frames.size(); c++) {
            if (matches_per_candidate[c].size() < n_cams) matches_per_candidate[c].resize(n_cams);
            for (size_t cam = 0; cam < n_cams; cam++) {
                add_job(descriptors[cam][frame], descriptors[cam][candidate_frames[c]]);
                out.push_back(&matches_per_candidate[c][cam]);
            }
        }
        run(out);
    }

private:
    template <typename Mat>
    const uint8_t* rows_of(const Mat& m, int32_t* n) {
        *n = (int32_t)m.rows;
        if (m.rows <= 0) { *n = 0; return nullptr; }
        if (m.cols != 64) throw std::runtime_error("matchFeatures: descriptors must have 64 byte columns (FREAK), got " + std::to_string(m.cols));
        const uint8_t* p0 = (const uint8_t*)m.template ptr<unsigned char>(0);
        const uint8_t* pl = (const uint8_t*)m.template ptr<unsigned char>(m.rows - 1);
        if (pl == p0 + 64 * (size_t)(m.rows - 1)) return p0;                       // contiguous: passed as it is
        std::map<const uint8_t*, size_t>::const_iterator it = gathered_.find(p0);   // a ROI: gathered once per call
        if (it != gathered_.end() && bufs_[it->second].size() == 64 * (size_t)m.rows) return bufs_[it->second].data();
        bufs_.push_back(std::vector<uint8_t>(64 * (size_t)m.rows));
        for (int r = 0; r < m.rows; r++) std::memcpy(&bufs_.back()[64 * (size_t)r], (const uint8_t*)m.template ptr<unsigned char>(r), 64);
        gathered_[p0] = bufs_.size() - 1;
        return bufs_.back().data();
    }
    void begin() { jobs_.clear(); bufs_.clear(); gathered_.clear(); }
    template <typename Mat>
    void add_job(const Mat& query, const Mat& train) {
        velo_desc_job j;
        j.query = rows_of(query, &j.n_query);
        j.train = rows_of(train, &j.n_train);
        jobs_.push_back(j);
    }
    void run(const std::vector<std::vector<std::pair<int, int> >*>& out) {
        size_t nq = 0;
        for (size_t j = 0; j < jobs_.size(); j++) nq += (size_t)jobs_[j].n_query;
        idx_.resize(nq + 1); dist_.resize(nq + 1); pairs_.resize(2 * nq + 2);
        md_.resize(jobs_.size() + 1); nk_.resize(jobs_.size() + 1);
        const int s = velo_match_descriptors(ctx_, jobs_.data(), (int32_t)jobs_.size(), match_thresh_, idx_.data(), dist_.data(), md_.data(),
                                             nk_.data(), pairs_.data());
        bufs_.clear(); gathered_.clear();
        if (s != VELO_OK) throw std::runtime_error(std::string("velo_match_descriptors: ") + velo_last_error());
        size_t w = 0;
        for (size_t j = 0; j < jobs_.size(); j++)
            for (int k = 0; k < nk_[j]; k++, w++) out[j]->push_back(std::make_pair((int)pairs_[2 * w], (int)pairs_[2 * w + 1]));   // velo.h:547
    }

    velo_ctx* ctx_;
    double match_thresh_;
    std::vector<velo_desc_job> jobs_;
    std::vector<std::vector<uint8_t> > bufs_;
    std::map<const uint8_t*, size_t> gathered_;
    std::vector<int32_t> idx_, dist_, md_, nk_, pairs_;
};

// velo.h:562-579 (host code, as in the reference: the last index of a repeated id in frame1 wins, frame2's order is kept)
inline void matchUsingId(const std::vector<std::vector<std::vector<int> > >& keypoint_ids, const int cam1, const int cam2, const int frame1,
                         const int frame2, std::vector<std::pair<int, int> >& matches) {
    std::map<int, int> id2ind;
    for (int ind = 0; ind < (int)keypoint_ids[cam1][frame1].size(); ind++) id2ind[keypoint_ids[cam1][frame1][ind]] = ind;
    for (int ind = 0; ind < (int)keypoint_ids[cam2][frame2].size(); ind++) {
        const int id = keypoint_ids[cam2][frame2][ind];
        std::map<int, int>::const_iterator it = id2ind.find(id);
        if (it != id2ind.end()) matches.push_back(std::make_pair(it->second, ind));
    }
}

// velo.h:580-590
inline void matchUsingId(const std::vector<std::vector<std::vector<int> > >& keypoint_ids, const int frame1, const int frame2,
                         std::vector<std::vector<std::pair<int, int> > >& matches) {
    for (size_t cam = 0; cam < keypoint_ids.size(); cam++) matchUsingId(keypoint_ids, (int)cam, (int)cam, frame1, frame2, matches.at(cam));
}

}  // namespace velo_hip

#endif  // VELO_MATCH_FEATURES_HPP_
