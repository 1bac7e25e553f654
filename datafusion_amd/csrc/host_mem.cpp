// Pinned host memory: the C API that gives callers DMA-able buffers
// (dfmi_host_alloc / _free / _register / _unregister) with its registry, the
// recycling pool of result blocks, and dfmi_host_result's accessors.
#include "host_mem.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "buffers.h"

using dfmi::Fail;
using dfmi::xi::set_err;

namespace dfmi {
namespace host {

PinnedPool::PinnedPool() {
    if (const char* e = getenv("DFMI_HOST_POOL_MB")) limit_ = (size_t)std::max(0ll, atoll(e)) << 20;
}

PinnedPool::~PinnedPool() {
    for (auto& kv : free_) (void)hipHostFree(kv.second);
}

static size_t round_block(size_t b) {
    b = std::max<size_t>(b, 64);
    const size_t q = b < ((size_t)2 << 20) ? 4096 : ((size_t)2 << 20);
    return (b + q - 1) / q * q;
}

PinnedPool::Blk PinnedPool::get(size_t bytes) {
    const size_t cap = round_block(bytes);
    {
        std::lock_guard<std::mutex> g(m_);
        auto it = free_.lower_bound(cap);
        if (it != free_.end() && it->first <= 2 * cap + ((size_t)2 << 20)) {
            Blk b{(uint8_t*)it->second, it->first};
            free_bytes_ -= it->first;
            free_.erase(it);
            return b;
        }
    }
    void* p = nullptr;
    if (hipHostMalloc(&p, cap, hipHostMallocDefault) != hipSuccess) {
        (void)hipGetLastError();
        {
            std::lock_guard<std::mutex> g(m_);
            trim(0);
        }
        const hipError_t e = hipHostMalloc(&p, cap, hipHostMallocDefault);
        if (e != hipSuccess) throw Fail{DFMI_ERR_DEVICE, std::string("hipHostMalloc (result): ") + hipGetErrorString(e)};
    }
    return {(uint8_t*)p, cap};
}

void PinnedPool::recycle(Blk& b) {
    std::lock_guard<std::mutex> g(m_);
    free_.emplace(b.cap, b.p);
    free_bytes_ += b.cap;
    b = Blk{};
    trim(limit_);
}

void PinnedPool::trim(size_t limit) {
    while (free_bytes_ > limit && !free_.empty()) {
        auto it = std::prev(free_.end());
        free_bytes_ -= it->first;
        (void)hipHostFree(it->second);
        free_.erase(it);
    }
}

namespace {
// Ranges the DMA engines can read directly: dfmi_host_alloc'd or
// dfmi_host_register'd. Process-wide (a buffer may feed any context).
struct PinRegistry {
    std::mutex m;
    std::map<uintptr_t, std::pair<size_t, bool>> r;  // base -> (bytes, registered (vs allocated))
};
PinRegistry& pins() {
    static PinRegistry* p = new PinRegistry();
    return *p;
}
// Pinned by the runtime (hipHostMalloc'd elsewhere, e.g. a torch pinned
// tensor): asked only for large buffers, whose staging copy would matter.
bool runtime_pinned(const void* p) {
    hipPointerAttribute_t a;
    const hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) {
        (void)hipGetLastError();  // pageable memory: not an error of this call
        return false;
    }
    return a.type == hipMemoryTypeHost;
}
// Takes p out of the registry if it is there as `registered`.
bool unpin(void* p, bool registered) {
    PinRegistry& R = pins();
    std::lock_guard<std::mutex> g(R.m);
    auto it = R.r.find((uintptr_t)p);
    if (it == R.r.end() || it->second.second != registered) return false;
    R.r.erase(it);
    return true;
}
}  // namespace

bool is_pinned(const void* p, size_t n) {
    if (!p || !n) return false;
    {
        PinRegistry& R = pins();
        std::lock_guard<std::mutex> g(R.m);
        auto it = R.r.upper_bound((uintptr_t)p);
        if (it != R.r.begin()) {
            --it;
            if ((uintptr_t)p + n <= it->first + it->second.first) return true;
        }
    }
    return n >= ((size_t)1 << 20) && runtime_pinned(p) && runtime_pinned((const uint8_t*)p + n - 1);
}

}  // namespace host
}  // namespace dfmi

using dfmi::host::pins;
using dfmi::host::PinRegistry;

extern "C" int32_t dfmi_host_alloc(size_t bytes, void** out, dfmi_error* err) {
    set_err(err, DFMI_OK, "");
    if (!out) {
        set_err(err, DFMI_ERR_INVALID_ARGUMENT, "out is NULL");
        return DFMI_ERR_INVALID_ARGUMENT;
    }
    *out = nullptr;
    void* p = nullptr;
    const hipError_t e = hipHostMalloc(&p, std::max<size_t>(bytes, 64), hipHostMallocPortable);
    if (e != hipSuccess) {
        set_err(err, DFMI_ERR_DEVICE, std::string("hipHostMalloc: ") + hipGetErrorString(e));
        return DFMI_ERR_DEVICE;
    }
    {
        PinRegistry& R = pins();
        std::lock_guard<std::mutex> g(R.m);
        R.r[(uintptr_t)p] = {std::max<size_t>(bytes, 64), false};
    }
    *out = p;
    return DFMI_OK;
}

extern "C" int32_t dfmi_host_free(void* p) {
    if (!p) return DFMI_OK;
    if (!dfmi::host::unpin(p, false)) return DFMI_ERR_INVALID_ARGUMENT;
    return hipHostFree(p) == hipSuccess ? DFMI_OK : DFMI_ERR_DEVICE;
}

extern "C" int32_t dfmi_host_register(void* p, size_t bytes, dfmi_error* err) {
    set_err(err, DFMI_OK, "");
    if (!p || !bytes) {
        set_err(err, DFMI_ERR_INVALID_ARGUMENT, "NULL or empty range");
        return DFMI_ERR_INVALID_ARGUMENT;
    }
    const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterPortable);
    if (e != hipSuccess) {
        set_err(err, DFMI_ERR_DEVICE, std::string("hipHostRegister: ") + hipGetErrorString(e));
        return DFMI_ERR_DEVICE;
    }
    PinRegistry& R = pins();
    std::lock_guard<std::mutex> g(R.m);
    R.r[(uintptr_t)p] = {bytes, true};
    return DFMI_OK;
}

extern "C" int32_t dfmi_host_unregister(void* p) {
    if (!p || !dfmi::host::unpin(p, true)) return DFMI_ERR_INVALID_ARGUMENT;
    return hipHostUnregister(p) == hipSuccess ? DFMI_OK : DFMI_ERR_DEVICE;
}

// ---------------------------------------------------------------- results
extern "C" int32_t dfmi_host_result_num_columns(const dfmi_host_result* r) { return r ? (int32_t)r->cols.size() : 0; }

extern "C" int32_t dfmi_host_result_column(const dfmi_host_result* r, int32_t i, dfmi_column* view) {
    if (!r || !view || i < 0 || i >= (int32_t)r->cols.size()) return DFMI_ERR_INVALID_ARGUMENT;
    const dfmi_host_result::Col& c = r->cols[i];
    memset(view, 0, sizeof *view);
    view->type = c.type;
    view->length = c.length;
    view->null_count = c.null_count;
    view->validity = c.has_validity ? c.validity.data() : nullptr;
    view->values = c.type == DFMI_TYPE_BOOLEAN && !c.values.p ? (const void*)c.bits.data() : (const void*)c.values.p;
    view->offsets = c.type == DFMI_TYPE_UTF8 ? (const int32_t*)c.offsets.p : nullptr;
    if (c.v_values || c.v_offsets) {  // batches form
        view->values = c.v_values;
        view->offsets = c.type == DFMI_TYPE_UTF8 ? c.v_offsets : nullptr;
        view->validity = c.null_count > 0 ? c.v_validity : nullptr;
    }
    return DFMI_OK;
}

extern "C" int32_t dfmi_host_result_columns(const dfmi_host_result* r, int32_t first, int32_t count,
                                            dfmi_column* views) {
    if (!r || !views || first < 0 || count < 0 || (int64_t)first + count > (int64_t)r->cols.size())
        return DFMI_ERR_INVALID_ARGUMENT;
    for (int32_t k = 0; k < count; ++k) dfmi_host_result_column(r, first + k, &views[k]);
    return DFMI_OK;
}

extern "C" int32_t dfmi_host_result_block(const dfmi_host_result* r, const void** base, size_t* bytes) {
    if (!r || !base || !bytes) return DFMI_ERR_INVALID_ARGUMENT;
    *base = r->arena.p;
    *bytes = r->arena.p ? r->arena.cap : 0;
    return DFMI_OK;
}

extern "C" void dfmi_host_result_free(dfmi_host_result* r) { delete r; }
