// Minimal stand-in for the one OpenCV type the descriptor-matching adaptor (include/velo_match_features.hpp) needs: a matrix of
// 8-bit rows with rows, cols and ptr<T>(r), like cv::Mat.  The row stride may exceed cols, as in a cv::Mat ROI, so that the
// adaptor's gather path is exercised too.  No reference source is compiled against it.
#pragma once
#include <vector>

namespace standin {
struct Mat {
    int rows, cols, step;
    std::vector<unsigned char> data;
    Mat() : rows(0), cols(0), step(0) {}
    Mat(int r, int c, int s) : rows(r), cols(c), step(s), data((size_t)(r > 0 ? r : 0) * (size_t)s, 0) {}
    template <typename T> T* ptr(int r) { return (T*)(data.data() + (size_t)r * step); }
    template <typename T> const T* ptr(int r) const { return (const T*)(data.data() + (size_t)r * step); }
};
}  // namespace standin
