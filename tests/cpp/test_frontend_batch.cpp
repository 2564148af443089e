// Drives the batch members of include/velo_track_features.hpp and include/velo_detect_features.hpp (several sequences, one tracker /
// detector and one context each, ONE library call per stage) next to the single-sequence members, against the stand-in types of
// track_standin.hpp.  Needs the GPU.
// Input (argv[1]): n_seq, n_cams, the first id; then per sequence: width, height, the previous then the current image of every camera, K
// and Kinv of every camera, then per camera: n, n pixel points, n ids, n x 64 descriptor bytes (frame 0).
// Run twice over the same input on fresh contexts: "single" -- per sequence setImages twice, trackFeaturesFrame into frame 1,
// detectFeaturesFrame on frame 1 (the tracked points are the existing ones); "batch" -- setImagesBatch twice, trackFeaturesFrameBatch,
// detectFeaturesFrameBatch over all sequences.  After each stage the lists of frame 1 of every sequence and camera are printed
// (<mode>_track / <mode>_detect, sequence-major), then the id counters; the caller compares the two runs.
// The stand-in extractor DELETES every key point with (x + 3 y) % 5 == 0 and writes, for the k-th key point that is left, a 64-byte row
// that starts (x & 255, x >> 8, y & 255, y >> 8, 0xAB, k & 255, k >> 8, 0xCD, sequence).
// Output, one list per line: <name> <n> values (floats as their 32-bit patterns, ids, descriptor bytes).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "track_standin.hpp"
#include "velo_detect_features.hpp"
#include "velo_track_features.hpp"

using standin::Mat;
using standin::Matrix3f;
using standin::Point2f;
typedef std::vector<std::vector<std::vector<Point2f> > > Pts;
typedef std::vector<std::vector<std::vector<int> > > Ids;
typedef std::vector<std::vector<Mat> > Descs;
typedef velo_hip::FeatureTracker<Matrix3f> Tracker;
typedef velo_hip::CornerDetector<Matrix3f> Detector;

struct KeyPoint {
    Point2f pt;
    float size;
    KeyPoint(Point2f p, float s) : pt(p), size(s) {}
};

struct Extractor {
    int seq;
    void compute(const standin::Image&, std::vector<KeyPoint>& kps, Mat& out) const {
        std::vector<KeyPoint> left;
        for (size_t i = 0; i < kps.size(); i++)
            if (((int)kps[i].pt.x + 3 * (int)kps[i].pt.y) % 5 != 0) left.push_back(kps[i]);
        kps = left;
        out = Mat((int)kps.size(), 64, 0);
        for (size_t k = 0; k < kps.size(); k++) {
            const int x = (int)kps[k].pt.x, y = (int)kps[k].pt.y;
            unsigned char* r = &out.bytes[k * 64];
            r[0] = (unsigned char)(x & 255); r[1] = (unsigned char)(x >> 8); r[2] = (unsigned char)(y & 255); r[3] = (unsigned char)(y >> 8);
            r[4] = 0xAB; r[5] = (unsigned char)(k & 255); r[6] = (unsigned char)(k >> 8); r[7] = 0xCD; r[8] = (unsigned char)seq;
        }
    }
};

struct Sequence {
    int w, h;
    std::vector<standin::Image> prev, cur;
    std::vector<Matrix3f> K, Kinv;
    Pts kp, kp_p;
    Ids ids;
    Descs desc;
};

static FILE* g_in = 0;
static void rd(void* p, size_t n) { if (n && std::fread(p, 1, n, g_in) != n) { std::fprintf(stderr, "short input\n"); std::exit(2); } }
static int rd_i() { int v; rd(&v, 4); return v; }
static unsigned bits(float f) { unsigned u; std::memcpy(&u, &f, 4); return u; }

static void print_lists(const std::string& name, const std::vector<Point2f>& k, const std::vector<Point2f>& p, const std::vector<int>& ids,
                        const Mat& d) {
    std::printf("%s_k %d", name.c_str(), (int)k.size());
    for (size_t i = 0; i < k.size(); i++) std::printf(" %u %u", bits(k[i].x), bits(k[i].y));
    std::printf("\n%s_p %d", name.c_str(), (int)p.size());
    for (size_t i = 0; i < p.size(); i++) std::printf(" %u %u", bits(p[i].x), bits(p[i].y));
    std::printf("\n%s_id %d", name.c_str(), (int)ids.size());
    for (size_t i = 0; i < ids.size(); i++) std::printf(" %d", ids[i]);
    std::printf("\n%s_d %d", name.c_str(), d.rows);
    for (size_t i = 0; i < d.bytes.size(); i++) std::printf(" %d", (int)d.bytes[i]);
    std::printf("\n");
}

static void print_all(const std::string& name, const std::vector<Sequence>& S, int n_cams) {
    for (size_t i = 0; i < S.size(); i++)
        for (int c = 0; c < n_cams; c++) print_lists(name, S[i].kp[c][1], S[i].kp_p[c][1], S[i].ids[c][1], S[i].desc[c][1]);
}

// one run over copies of the sequences; batch: the batch members, else the single-sequence members
static void run(std::vector<Sequence> S, int n_cams, int first_id, bool batch) {
    const size_t n = S.size();
    const std::string mode = batch ? "batch" : "single";
    std::vector<velo_ctx*> ctxs(n, (velo_ctx*)NULL);
    for (size_t i = 0; i < n; i++)
        if (velo_create(&ctxs[i], 0) != VELO_OK) throw std::runtime_error(std::string("velo_create: ") + velo_last_error());
    try {
        std::vector<Tracker> trackers;
        std::vector<Detector> detectors;
        std::vector<Extractor> ex(n);
        std::vector<int> counters(n), frames(n, 1);
        for (size_t i = 0; i < n; i++) {
            trackers.push_back(Tracker(ctxs[i], S[i].K, S[i].Kinv));
            detectors.push_back(Detector(ctxs[i], S[i].Kinv));
            ex[i].seq = (int)i;
            counters[i] = first_id + 10000 * (int)i;
        }
        if (!batch) {
            for (size_t i = 0; i < n; i++) {
                trackers[i].setImages(S[i].prev);
                trackers[i].setImages(S[i].cur);
                trackers[i].trackFeaturesFrame(S[i].kp, S[i].kp_p, S[i].ids, S[i].desc, 1);
            }
            print_all(mode + "_track", S, n_cams);
            for (size_t i = 0; i < n; i++) {
                const Extractor* e = &ex[i];
                detectors[i].detectFeaturesFrame<KeyPoint>(S[i].kp, S[i].kp_p, S[i].ids, S[i].desc, e, S[i].cur, counters[i], 1);
            }
        } else {
            std::vector<Tracker*> tp;
            std::vector<Detector*> dp;
            std::vector<std::vector<standin::Image> > prev, cur;
            std::vector<Pts*> kp, kp_p;
            std::vector<Ids*> ids;
            std::vector<Descs*> desc;
            std::vector<const Extractor*> ep;
            std::vector<int*> cp;
            for (size_t i = 0; i < n; i++) {
                tp.push_back(&trackers[i]); dp.push_back(&detectors[i]);
                prev.push_back(S[i].prev); cur.push_back(S[i].cur);
                kp.push_back(&S[i].kp); kp_p.push_back(&S[i].kp_p); ids.push_back(&S[i].ids); desc.push_back(&S[i].desc);
                ep.push_back(&ex[i]); cp.push_back(&counters[i]);
            }
            Tracker::setImagesBatch(tp, prev);
            Tracker::setImagesBatch(tp, cur);
            Tracker::trackFeaturesFrameBatch(tp, kp, kp_p, ids, desc, frames);
            print_all(mode + "_track", S, n_cams);
            Detector::detectFeaturesFrameBatch<KeyPoint>(dp, kp, kp_p, ids, desc, ep, cur, cp, frames);
        }
        print_all(mode + "_detect", S, n_cams);
        std::printf("%s_counters %d", mode.c_str(), (int)n);
        for (size_t i = 0; i < n; i++) std::printf(" %d", counters[i]);
        std::printf("\n");
    } catch (...) {
        for (size_t i = 0; i < n; i++) velo_destroy(ctxs[i]);
        throw;
    }
    for (size_t i = 0; i < n; i++) velo_destroy(ctxs[i]);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    g_in = std::fopen(argv[1], "rb");
    if (!g_in) return 2;
    const int n_seq = rd_i(), n_cams = rd_i(), first_id = rd_i();
    std::vector<Sequence> S(n_seq);
    for (int s = 0; s < n_seq; s++) {
        Sequence& Q = S[s];
        Q.w = rd_i(); Q.h = rd_i();
        for (int pass = 0; pass < 2; pass++)
            for (int c = 0; c < n_cams; c++) {
                standin::Image im(Q.h, Q.w, (size_t)Q.w + 3 + s);         // padded rows, a different stride per sequence
                for (int y = 0; y < Q.h; y++) rd(im.data + (size_t)y * im.step, (size_t)Q.w);
                (pass ? Q.cur : Q.prev).push_back(im);
            }
        Q.K.resize(n_cams); Q.Kinv.resize(n_cams);
        for (int c = 0; c < n_cams; c++) { rd(Q.K[c].v, 36); rd(Q.Kinv[c].v, 36); }
        Q.kp.assign(n_cams, std::vector<std::vector<Point2f> >(2)); Q.kp_p = Q.kp;
        Q.ids.assign(n_cams, std::vector<std::vector<int> >(2));
        Q.desc.assign(n_cams, std::vector<Mat>(2));
        for (int c = 0; c < n_cams; c++) {
            const int n = rd_i();
            for (int i = 0; i < n; i++) {
                Point2f p;
                rd(&p.x, 4); rd(&p.y, 4);
                Q.kp_p[c][0].push_back(p);
                Q.kp[c][0].push_back(velo_hip::pixel2canonical(p, Q.Kinv[c]));
            }
            for (int i = 0; i < n; i++) Q.ids[c][0].push_back(rd_i());
            Q.desc[c][0] = Mat(n, 64, 0);
            rd(Q.desc[c][0].bytes.data(), Q.desc[c][0].bytes.size());
        }
    }
    std::fclose(g_in);
    try {
        run(S, n_cams, first_id, false);
        run(S, n_cams, first_id, true);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 4;
    }
    return 0;
}
