// Owners of device and pinned host memory, and the HIP error check. Every
// grow-only buffer of the library is one of these two; a site's growth policy
// (exact size, a floor, 25 % slack) is an argument of the grow call.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <string>
#include <utility>

#include "abi_guard.h"

#define HIP_TRY(x)                                                                        \
    do {                                                                                   \
        hipError_t e_ = (x);                                                               \
        if (e_ != hipSuccess) throw dfmi::Fail{DFMI_ERR_DEVICE, std::string(#x ": ") + hipGetErrorString(e_)}; \
    } while (0)

namespace dfmi {

// What a buffer that must grow allocates for `want` units: at least `floor`,
// plus want / slack_div of headroom (0: none).
struct Grow {
    size_t floor = 0;
    int slack_div = 0;
    size_t of(size_t want) const {
        want = std::max(want, floor);
        return want + (slack_div ? want / (size_t)slack_div : 0);
    }
};
constexpr Grow kGrowExact{0, 0};
constexpr Grow kGrowScratch{64, 4};  // a scratch buffer: 64 at the least, 25 % slack

// Pinned host memory that keeps its capacity (a finish's copies land here by
// DMA; no zero-fill, no page faults once warm). `dev` is the device's address
// of the block (kernels that read or write it in place).
template <typename T>
struct HostBuf {
    T* p = nullptr;
    T* dev = nullptr;
    size_t n = 0, cap = 0;
    HostBuf() = default;
    HostBuf(const HostBuf&) = delete;
    HostBuf& operator=(const HostBuf&) = delete;
    ~HostBuf() {
        if (p) (void)hipHostFree(p);
    }
    // `want` elements, contents dropped when the block has to grow.
    void resize(size_t want, Grow g = {16, 4}) {
        if (want > cap) {
            if (p) (void)hipHostFree(p);
            p = dev = nullptr;
            cap = 0;
            const size_t c = g.of(want);
            HIP_TRY(hipHostMalloc((void**)&p, c * sizeof(T), hipHostMallocDefault));
            cap = c;
            HIP_TRY(hipHostGetDevicePointer((void**)&dev, p, 0));
        }
        n = want;
    }
    T* data() { return p; }
    const T* data() const { return p; }
    size_t size() const { return n; }
    T& operator[](size_t i) { return p[i]; }
    const T& operator[](size_t i) const { return p[i]; }
};

// Device memory with one owner (move-only; freed with it).
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;  // bytes
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr, o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        std::swap(p, o.p);
        std::swap(cap, o.cap);
        return *this;
    }
    ~DevBuf() {
        if (p) (void)hipFree(p);
    }
    template <typename T>
    T* as() const { return (T*)p; }
    // A block of exactly `bytes` (the old one freed first, its contents dropped).
    void alloc(size_t bytes) {
        if (p) HIP_TRY(hipFree(p));
        p = nullptr;
        cap = 0;
        HIP_TRY(hipMalloc(&p, bytes));
        cap = bytes;
    }
    // At least `bytes`: a buffer that keeps its capacity, contents dropped
    // when it has to grow.
    void* reserve(size_t bytes, Grow g = kGrowScratch) {
        bytes = std::max(bytes, g.floor);
        if (cap < bytes) alloc(g.of(bytes));
        return p;
    }
    // A block of `want` bytes with the first `keep` bytes copied over.
    void regrow(hipStream_t stream, size_t keep, size_t want) {
        DevBuf q;
        q.alloc(want);
        if (keep) HIP_TRY(hipMemcpyAsync(q.p, p, keep, hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        *this = std::move(q);  // (the old block goes with q)
    }
};

}  // namespace dfmi
