// velo_scan_map.hpp -- header-only C++11 owner of a device-resident scan map (velo_map_*, include/velo_hip.h): the sliding window of
// scan-to-map odometry, every scan kept as it was registered with its pose, the target cloud written on demand in the frame the caller
// names.  Plain pointers and std::vector only; every member returns the C-ABI's status (VELO_OK == 0) and velo_last_error() has the text.
//
//     velo_hip::ScanMap map(0, 17, 2100000);
//     map.load(ctx, inverse_of_newest_pose);             // the window becomes ctx's target, in the newest pose's frame
//     velo_frame_to_frame(ctx, x, T, &summary);          // ctx's source: the new scan
//     map.insert(ctx, false, frame, new_pose);           // the scan enters the window, device to device; the oldest one leaves
#ifndef VELO_SCAN_MAP_HPP_
#define VELO_SCAN_MAP_HPP_

#include <cstddef>
#include <vector>

#include "velo_hip.h"

namespace velo_hip {

class ScanMap {
public:
    struct Info { int64_t scans, points, rings, max_scans, max_points, evictions, arena_points, arena_growths; };

    ScanMap(int device, int max_scans, int64_t max_points) : h_(0), status_(velo_map_create(&h_, device, max_scans, max_points)) {}
    ~ScanMap() { velo_map_destroy(h_); }

    int status() const { return status_; }                 // of the constructor's velo_map_create
    velo_map* get() const { return h_; }

    // the scan ctx holds (its source, or its whole-scan target) enters under `frame`; *n_evicted: the oldest scans that went for it
    int insert(velo_ctx* ctx, bool of_target, int frame, const double pose16[16], int* n_evicted = 0) {
        int32_t gone = 0;
        const int st = velo_map_insert(h_, ctx, of_target ? 1 : 0, frame, pose16, &gone);
        if (n_evicted) *n_evicted = gone;
        return st;
    }
    int set_pose(int frame, const double pose16[16]) { return velo_map_set_pose(h_, frame, pose16); }
    int drop(int frame) { return velo_map_drop(h_, frame); }
    int clear() { return velo_map_clear(h_); }

    std::vector<int> frames() const {                      // oldest first
        std::vector<int32_t> f((size_t)velo_map_frames(h_, 0, 0) + 1);
        const int n = velo_map_frames(h_, &f[0], (int32_t)f.size());
        return std::vector<int>(f.begin(), f.begin() + n);
    }
    int info(Info* out) const {
        int64_t v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        const int st = velo_map_info(h_, v);
        out->scans = v[0]; out->points = v[1]; out->rings = v[2]; out->max_scans = v[3]; out->max_points = v[4];
        out->evictions = v[5]; out->arena_points = v[6]; out->arena_growths = v[7];
        return st;
    }
    // one stored scan: xyz (n x 3), its ring offsets (n_rings + 1), its pose
    int get_scan(int frame, std::vector<float>* xyz, std::vector<int>* ring_offsets, double pose16[16]) const {
        int32_t n = 0, r = 0;
        int st = velo_map_get_scan(h_, frame, 0, 0, &n, 0, 0, &r, 0);
        if (st != VELO_OK) return st;
        std::vector<float> p(3 * (size_t)n + 3);
        std::vector<int32_t> off((size_t)r + 1);
        st = velo_map_get_scan(h_, frame, &p[0], n, &n, &off[0], r + 1, &r, pose16);
        if (st != VELO_OK) return st;
        p.resize(3 * (size_t)n);
        if (xyz) xyz->swap(p);
        if (ring_offsets) ring_offsets->assign(off.begin(), off.end());
        return VELO_OK;
    }
    // the window becomes ctx's target in the frame ref_inv16 (the INVERSE of the reference pose, row-major 4 x 4)
    int load(velo_ctx* ctx, const double ref_inv16[16]) { return velo_map_load(h_, ctx, ref_inv16); }

    // maps[i] -> ctxs[i] in the frame ref_inv[16 i ..], one materialise launch for all of them
    static int load_batch(const std::vector<ScanMap*>& maps, const std::vector<velo_ctx*>& ctxs, const std::vector<double>& ref_inv) {
        if (maps.empty() || maps.size() != ctxs.size() || ref_inv.size() != 16 * maps.size()) return VELO_ERR_INVALID;
        std::vector<velo_map*> m(maps.size());
        std::vector<velo_ctx*> c(ctxs);
        for (size_t i = 0; i < maps.size(); i++) m[i] = maps[i] ? maps[i]->h_ : 0;
        return velo_map_load_batch(&m[0], &c[0], (int32_t)m.size(), &ref_inv[0]);
    }

private:
    ScanMap(const ScanMap&);                               // one owner
    ScanMap& operator=(const ScanMap&);
    velo_map* h_;
    int status_;
};

}  // namespace velo_hip

#endif  // VELO_SCAN_MAP_HPP_
