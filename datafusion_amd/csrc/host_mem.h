// Pinned host memory of the host paths: the recycling pool that results are
// made of, the result type the C ABI hands out, and the registry of caller
// memory the DMA engines can read directly (host_mem.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <utility>
#include <vector>

#include "../../include/dfmi.h"

namespace dfmi {
namespace host {

// Allocator whose resize() leaves bytes uninitialised: result buffers are
// overwritten by the chunk copies, and zero-filling GBs first costs as much
// as the copy itself (untouched pages of a worst-case reservation are never
// faulted in).
template <class T>
struct uninit_alloc : std::allocator<T> {
    using std::allocator<T>::allocator;
    template <class U>
    struct rebind {
        using other = uninit_alloc<U>;
    };
    template <class U>
    void construct(U* p) noexcept {
        ::new ((void*)p) U;
    }
    template <class U, class... Args>
    void construct(U* p, Args&&... a) {
        ::new ((void*)p) U(std::forward<Args>(a)...);
    }
};

// Pinned host blocks that hold results, recycled across calls: a result's
// buffers are the DMA target of the D2H copies (no staging copy-out), and a
// freed result's blocks serve the next call -- fresh pageable buffers would
// cost a page fault per 4 KiB on first touch and a TLB shootdown per page on
// free, which measured slower than PCIe itself. Shared by a
// context and the results it made (a result may outlive its context).
class PinnedPool {
   public:
    struct Blk {
        uint8_t* p = nullptr;
        size_t cap = 0;
    };
    PinnedPool();  // DFMI_HOST_POOL_MB: idle pinned bytes kept for reuse
    ~PinnedPool();
    Blk get(size_t bytes);  // throws Fail
    void put(Blk& b) {  // (inline: a result frees two per column, most of them empty)
        if (b.p) recycle(b);
    }

   private:
    void recycle(Blk& b);
    void trim(size_t limit);  // largest blocks first
    std::mutex m_;
    std::multimap<size_t, void*> free_;
    size_t free_bytes_ = 0;
    size_t limit_ = (size_t)8 << 30;
};

// p .. p + n lies in memory the DMA engines can read: dfmi_host_alloc'd,
// dfmi_host_register'd, or (asked only for >= 1 MiB) pinned by the runtime.
bool is_pinned(const void* p, size_t n);

}  // namespace host
}  // namespace dfmi

struct dfmi_host_result {
    using Blk = dfmi::host::PinnedPool::Blk;
    using Bytes = std::vector<uint8_t, dfmi::host::uninit_alloc<uint8_t>>;
    struct Col {
        int32_t type = 0;
        int64_t length = 0, null_count = 0, data_length = 0;
        Blk values, offsets;  // fixed-width / Utf8 bytes; Utf8 offsets
        Bytes bits;           // Boolean values
        Bytes validity;
        bool has_validity = false;
        // dfmi_filter_project_host_batches: views into the result's arena
        const uint8_t* v_values = nullptr;
        const int32_t* v_offsets = nullptr;
        const uint8_t* v_validity = nullptr;
    };
    std::shared_ptr<dfmi::host::PinnedPool> pool;
    std::vector<Col> cols;
    Blk arena;  // one block holding every column (batches form)
    ~dfmi_host_result() {
        if (pool) {
            for (Col& c : cols) {
                pool->put(c.values);
                pool->put(c.offsets);
            }
            pool->put(arena);
        }
    }
};
