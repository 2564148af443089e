// The bookkeeping of the frame store's arenas (csrc/velo_block_list.h) on its own: no device, no library.
// (a) the put / drop sequences of the GPU state tests (test_gpu_visual_assembly.py::test_frame_store, test_gpu_loop_matches.py::test_state)
//     replayed through both arenas, with every entries / arena_bytes / arena_used / arena_reallocations / free_blocks assertion they make;
// (b) a seeded random sequence with the invariants checked after every step.
#include "velo_block_list.h"

#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>

using velo::Block;
using velo::BlockList;

#define CHECK(cond)                                                                   \
    do {                                                                              \
        if (!(cond)) { std::printf("%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); std::exit(1); } \
    } while (0)

namespace {

// what FrArena and a directory do with the list, without the device: grow == false stands for a reallocation that failed
struct Arena {
    BlockList L;
    std::map<int, Block> dir;
    size_t unit_bytes;
    Arena(size_t cap, size_t unit) : unit_bytes(unit) { L.cap = cap; }
    bool put(int key, size_t need, bool grow = true) {
        auto it = dir.find(key);
        const Block* old = it != dir.end() ? &it->second : nullptr;
        const BlockList::Plan p = L.plan(old, need);
        if (p.grow_to > 0) {
            if (!grow) return false;
            L.grew(p);
        }
        L.commit(p, old);
        dir[key] = p.block;
        return true;
    }
    void drop(int key) {
        auto it = dir.find(key);
        if (it == dir.end()) return;
        L.release(it->second);
        dir.erase(it);
    }
    struct Info {
        size_t entries, arena_bytes, arena_used, free_blocks; int reallocs;
        bool operator==(const Info& o) const {
            return entries == o.entries && arena_bytes == o.arena_bytes && arena_used == o.arena_used && free_blocks == o.free_blocks && reallocs == o.reallocs;
        }
    };
    Info info() const { return Info{dir.size(), L.cap * unit_bytes, L.used * unit_bytes, L.free_blocks.size(), L.reallocs}; }
};

int key(int frame, int cam) { return frame * 8 + cam; }
size_t words(int n, int n_with_depth) { return ((size_t)(4 * n + 3 * n_with_depth) + 15) / 16 * 16; }   // velo_frames_put: rounded to 16

// the store of velo_api_frames.inl: keypoint words and descriptor rows; putting keypoints drops the entry's rows
struct Store {
    Arena kp, rows;
    explicit Store(size_t arena_capacity) : kp((arena_capacity + 3) / 4, 4), rows((arena_capacity + 63) / 64, 64) {}
    void put(int frame, int cam, int n, int n_wd) { CHECK(kp.put(key(frame, cam), words(n, n_wd))); rows.drop(key(frame, cam)); }
    void put_rows(int frame, int cam, int n) { CHECK(kp.dir.count(key(frame, cam))); CHECK(rows.put(key(frame, cam), (size_t)n)); }
    void drop(int frame) { for (int cam = 0; cam < 2; cam++) { kp.drop(key(frame, cam)); rows.drop(key(frame, cam)); } }
};

struct Cam { int n, n_wd; };

// test_gpu_visual_assembly.py::test_frame_store; the depth counts are those its generator (seed 6) draws
void replay_frame_store() {
    Store S(4096);                                                   // 1,024 words
    const Cam f3[2] = {{200, 110}, {100, 39}}, f1[2] = {{150, 83}, {0, 0}}, f2[2] = {{300, 135}, {250, 136}};
    const Cam f2_small[2] = {{120, 59}, {40, 17}}, f2_large[2] = {{700, 374}, {650, 333}};
    auto put = [&](int f, const Cam* c) { for (int cam = 0; cam < 2; cam++) S.put(f, cam, c[cam].n, c[cam].n_wd); };
    put(3, f3); put(1, f1); put(2, f2);
    CHECK(S.kp.info().reallocs >= 2 && S.kp.info().entries == 6);
    CHECK(S.kp.dir.at(key(1, 1)).cap == 0);                           // the empty entry owns no block
    size_t used = S.kp.info().arena_used;
    put(2, f2_small);                                                // in place
    CHECK(S.kp.info().arena_used == used && S.kp.info().entries == 6);
    put(2, f2_large);                                                // moved: both outgrown blocks are free now
    CHECK(S.kp.info().arena_used > used && S.kp.info().free_blocks >= 2);
    S.drop(3);
    CHECK(S.kp.info().entries == 4);
    S.put(3, 0, f3[0].n, f3[0].n_wd);
    used = S.kp.info().arena_used;
    S.put(3, 1, f3[1].n, f3[1].n_wd);                                // a freed block is taken
    CHECK(S.kp.info().arena_used == used);
    CHECK(S.rows.info() == (Arena::Info{0, 4096, 0, 0, 0}));
}

// test_gpu_loop_matches.py::test_state; depth counts of its generator (seeds 15 and 16)
void replay_state() {
    Store S(4096);                                                   // 64 rows
    CHECK(S.rows.info() == (Arena::Info{0, 4096, 0, 0, 0}));
    const Cam fr[4][2] = {{{150, 67}, {90, 40}}, {{200, 104}, {100, 45}}, {{260, 129}, {70, 37}}, {{300, 143}, {0, 0}}};
    const int order[4] = {3, 0, 2, 1};
    for (int f : order) for (int cam = 0; cam < 2; cam++) S.put(f, cam, fr[f][cam].n, fr[f][cam].n_wd);
    const Arena::Info before = S.kp.info();
    for (int f : order) for (int cam = 1; cam >= 0; cam--) S.put_rows(f, cam, fr[f][cam].n);
    const Arena::Info info = S.rows.info();
    CHECK(info.entries == 8 && info.reallocs >= 2 && info.arena_bytes >= 64 * 1170);
    CHECK(S.kp.info() == before);                                    // the keypoint arena does not know of the rows
    for (int cam = 0; cam < 2; cam++) S.put_rows(0, cam, fr[0][cam].n);   // in place: the same size
    CHECK(S.rows.info() == info);
    S.put(1, 0, fr[1][0].n, fr[1][0].n_wd);                          // frames_put drops the rows
    CHECK(S.rows.info().entries == 7 && S.rows.info().free_blocks == info.free_blocks + 1);
    S.put_rows(1, 0, fr[1][0].n);                                    // the freed block is taken again
    CHECK(S.rows.info() == info);
    S.drop(2);
    CHECK(S.rows.info().entries == 6);
    for (int cam = 0; cam < 2; cam++) { S.put(2, cam, fr[2][cam].n, fr[2][cam].n_wd); S.put_rows(2, cam, fr[2][cam].n); }
    CHECK(S.rows.info().arena_bytes == info.arena_bytes);
    const Arena::Info keypoint_side = S.kp.info();
    for (int k = 0; k < 3; k++) S.put_rows(3, 0, fr[3][0].n);
    CHECK(S.kp.info() == keypoint_side);
    Store fresh(1u << 20);                                           // velo_frames_reset without a capacity
    CHECK(fresh.rows.info() == (Arena::Info{0, 1u << 20, 0, 0, 0}));
}

bool same(const Block& a, const Block& b) { return a.off == b.off && a.cap == b.cap; }

void check_layout(const Arena& A) {
    std::vector<Block> all(A.L.free_blocks);
    for (const auto& kv : A.dir) if (kv.second.cap > 0) all.push_back(kv.second);
    for (size_t i = 0; i < all.size(); i++) {
        CHECK(all[i].cap > 0 && all[i].off + all[i].cap <= A.L.used);
        for (size_t j = 0; j < i; j++) CHECK(all[i].off + all[i].cap <= all[j].off || all[j].off + all[j].cap <= all[i].off);
    }
    CHECK(A.L.used <= A.L.cap);
}

void random_sequence(unsigned seed, int steps) {
    std::mt19937 rng(seed);
    Arena A(256, 4);
    int n_in_place = 0, n_free = 0, n_front = 0, n_refused = 0, n_drop = 0;
    for (int step = 0; step < steps; step++) {
        const int k = (int)(rng() % 20);
        const Arena before = A;
        auto it = before.dir.find(k);
        const bool had = it != before.dir.end();
        const Block old = had ? it->second : Block();
        const size_t n_free_before = before.L.free_blocks.size();
        if (rng() % 4 == 0) {                                        // drop
            A.drop(k);
            CHECK(!A.dir.count(k) && A.L.used == before.L.used && A.L.cap == before.L.cap && A.L.reallocs == before.L.reallocs);
            CHECK(A.L.free_blocks.size() == n_free_before + (had && old.cap > 0 ? 1 : 0));
            if (had && old.cap > 0) CHECK(same(A.L.free_blocks.back(), old));
            n_drop += had;
        } else {
            const size_t need = rng() % 301;
            const bool grow = rng() % 4 == 0;
            // what has to happen, worked out here from the state before
            int want_free = -1;
            for (size_t f = 0; f < n_free_before && want_free < 0; f++) if (before.L.free_blocks[f].cap >= need) want_free = (int)f;
            const bool in_place = (had && old.cap >= need) || need == 0;
            const bool ok = A.put(k, need, grow);
            if (!ok) {                                               // the reallocation "failed": nothing has changed
                CHECK(!in_place && want_free < 0 && before.L.used + need > before.L.cap);
                CHECK(A.info() == before.info() && A.dir.size() == before.dir.size() && A.dir.count(k) == before.dir.count(k));
                if (had) CHECK(same(A.dir.at(k), old));
                for (size_t f = 0; f < n_free_before; f++) CHECK(same(A.L.free_blocks[f], before.L.free_blocks[f]));
                n_refused++;
            } else {
                const Block now = A.dir.at(k);
                if (in_place) {
                    CHECK(same(now, had ? old : Block()));
                    CHECK(A.info() == (Arena::Info{before.dir.size() + (had ? 0 : 1), before.info().arena_bytes, before.info().arena_used, n_free_before, before.L.reallocs}));
                    n_in_place++;
                } else if (want_free >= 0) {
                    CHECK(same(now, before.L.free_blocks[(size_t)want_free]) && now.cap >= need);
                    CHECK(A.L.used == before.L.used && A.L.cap == before.L.cap && A.L.reallocs == before.L.reallocs);
                    CHECK(A.L.free_blocks.size() == n_free_before - 1 + (old.cap > 0 ? 1 : 0));
                    n_free++;
                } else {
                    CHECK(now.off == before.L.used && now.cap == need && A.L.used == before.L.used + need);
                    if (before.L.used + need > before.L.cap) {
                        CHECK(A.L.cap == std::max(before.L.used + need, 2 * before.L.cap) && A.L.reallocs == before.L.reallocs + 1);
                    } else {
                        CHECK(A.L.cap == before.L.cap && A.L.reallocs == before.L.reallocs);
                    }
                    CHECK(A.L.free_blocks.size() == n_free_before + (old.cap > 0 ? 1 : 0));
                    n_front++;
                }
                if (!in_place && old.cap > 0) CHECK(same(A.L.free_blocks.back(), old));   // the outgrown block went to the list
            }
        }
        check_layout(A);
    }
    std::printf("seed %u: %d in place, %d from the free list, %d from the front, %d refused, %d drops, %d reallocations\n", seed, n_in_place, n_free,
                n_front, n_refused, n_drop, A.L.reallocs);
    CHECK(n_in_place > 100 && n_free > 100 && n_front > 20 && n_refused > 0 && n_drop > 100 && A.L.reallocs >= 2);   // every path was taken
}

}  // namespace

int main() {
    replay_frame_store();
    replay_state();
    random_sequence(1, 4000);
    random_sequence(2, 4000);
    std::printf("block list ok\n");
    return 0;
}
