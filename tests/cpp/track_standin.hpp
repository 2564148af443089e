// Minimal stand-ins for the OpenCV / Eigen types the feature-tracking adaptor (include/velo_track_features.hpp) needs: a float point, a
// 3 x 3 float matrix with m(i, j), an 8-bit image with rows, cols, step and data, and a descriptor matrix with rows, cols, type(),
// row(i), clone(), push_back and Mat(rows, cols, type), with cv::Mat's copying semantics for these uses.  No reference source is
// compiled against them.
#pragma once
#include <cstddef>
#include <vector>

namespace standin {
struct Point2f {
    float x, y;
    Point2f() : x(0), y(0) {}
    Point2f(float a, float b) : x(a), y(b) {}
};

struct Matrix3f {
    float v[9];
    float operator()(int i, int j) const { return v[3 * i + j]; }
};

struct Image {
    int rows, cols;
    size_t step;
    std::vector<unsigned char> buf;
    unsigned char* data;
    Image() : rows(0), cols(0), step(0), data(0) {}
    Image(int r, int c, size_t s) : rows(r), cols(c), step(s), buf((size_t)r * s), data(buf.empty() ? 0 : &buf[0]) {}
    Image(const Image& o) : rows(o.rows), cols(o.cols), step(o.step), buf(o.buf), data(buf.empty() ? 0 : &buf[0]) {}
    Image& operator=(const Image&) = delete;
};

struct Mat {                                  // rows of `cols` bytes, contiguous
    int rows, cols;
    std::vector<unsigned char> bytes;
    Mat() : rows(0), cols(0) {}
    Mat(int r, int c, int /*type*/) : rows(r), cols(c), bytes((size_t)r * c) {}
    int type() const { return 0; }
    Mat row(int i) const { Mat m(1, cols, 0); for (int k = 0; k < cols; k++) m.bytes[k] = bytes[(size_t)i * cols + k]; return m; }
    Mat clone() const { return *this; }
    void push_back(const Mat& m) {
        if (rows == 0 && cols == 0) cols = m.cols;
        bytes.insert(bytes.end(), m.bytes.begin(), m.bytes.end());
        rows += m.rows;
    }
    const unsigned char* ptr(int r) const { return &bytes[(size_t)r * cols]; }
};
}  // namespace standin
