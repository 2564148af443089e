// velo_block_list.h -- the bookkeeping of one arena of the resident frame store (velo_api_frames.inl), in the arena's units (words,
// rows).  Host-only and free of any HIP type: tests/cpp/test_block_list.cpp checks it on its own.  First-fit, no splitting or merging.
// Placing a block has two phases, so that a caller whose device work fails in between leaves everything as it was: plan() decides and
// changes nothing; grew() follows the reallocation plan() asked for; commit() runs after the last call that can fail.
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

namespace velo {

struct Block { size_t off = 0, cap = 0; };                  // cap == 0: no block (an empty entry owns none)

struct BlockList {
    size_t used = 0, cap = 0;                               // units handed out from the front / units before the arena reallocates
    int reallocs = 0;
    std::vector<Block> free_blocks;                         // dropped and outgrown blocks

    struct Plan {
        Block block;                                        // where the entry goes
        bool in_place = false;                              // it keeps the block it has (or needs none)
        int from_free = -1;                                 // else the index of the free block it takes, or -1: the front of the arena
        size_t grow_to = 0;                                 // non-zero: the arena has to hold this many units first
    };

    // old: the block the entry holds now, or null.  In place when it fits, else the first free block that is large enough, else the front.
    Plan plan(const Block* old, size_t need) const {
        Plan p;
        if (old && old->cap >= need) { p.block = *old; p.in_place = true; }
        else if (need == 0) { p.in_place = true; }
        else {
            for (size_t k = 0; k < free_blocks.size() && p.from_free < 0; k++) if (free_blocks[k].cap >= need) p.from_free = (int)k;
            if (p.from_free >= 0) p.block = free_blocks[(size_t)p.from_free];
            else {
                if (used + need > cap) p.grow_to = std::max(used + need, 2 * cap);
                p.block.off = used; p.block.cap = need;
            }
        }
        return p;
    }
    void grew(const Plan& p) { cap = p.grow_to; reallocs++; }
    void commit(const Plan& p, const Block* old) {
        if (p.in_place) return;
        if (p.from_free >= 0) free_blocks.erase(free_blocks.begin() + p.from_free);
        else used += p.block.cap;
        if (old) release(*old);                             // the outgrown block
    }
    void release(const Block& b) { if (b.cap > 0) free_blocks.push_back(b); }
};

}  // namespace velo
