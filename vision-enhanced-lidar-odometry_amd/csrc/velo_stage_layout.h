// velo_stage_layout.h -- where the tables of one staged buffer lie.  A launch set of the visual side sends its tables in ONE upload and
// reads its results back in ONE copy; such a buffer is described once, part after part, and the description gives the host pointer that
// fills a part, the device pointer a kernel is launched on and the byte count that is reserved and copied.  Host-only and free of any
// HIP type: tests/cpp/test_stage_layout.cpp checks it on its own.
#pragma once

#include <cstddef>

namespace velo {

struct StageLayout {
    size_t bytes = 0;                                       // the cursor; in the end what the call reserves and copies
    template <typename T>
    struct Part {                                           // n elements of T at byte offset off
        size_t off = 0, n = 0;
        T* in(void* base) const { return reinterpret_cast<T*>(static_cast<unsigned char*>(base) + off); }
        const T* in(const void* base) const { return reinterpret_cast<const T*>(static_cast<const unsigned char*>(base) + off); }
        size_t size() const { return sizeof(T) * n; }
        size_t end() const { return off + size(); }
    };
    size_t align(size_t a) { return bytes = (bytes + a - 1) / a * a; }   // the cursor on the next multiple of a
    // the next part starts at the cursor rounded up to `a` (1: packed behind its predecessor) and takes sizeof(T) * n
    template <typename T>
    Part<T> add(size_t n, size_t a = 64) {
        const Part<T> p{align(a), n};
        bytes = p.end();
        return p;
    }
};

}  // namespace velo
