// The per-context staging arena of the host paths (host_chunks.cpp,
// host_batches.cpp): grow-only device and pinned regions, the copy streams
// with their events, the host threads and the pool results are made of. One
// per context, created on first use (a context is driven by one host thread,
// context.rs:33) and destroyed with it.
#pragma once
#include <memory>

#include "exec_internal.h"
#include "host_mem.h"
#include "host_pool.h"

namespace dfmi {

constexpr int kSlots = 3;  // chunks in flight in the chunk pipeline

struct Arena {
    hipStream_t h2d = nullptr, d2h = nullptr;
    hipEvent_t h2d_done[kSlots] = {}, d2h_done[kSlots] = {}, kdone[kSlots] = {};
    bool slot_used[kSlots] = {};
    DevBuf dev;             // the chunk pipeline's slots: [inputs | outputs] each
    HostBuf<uint8_t> pin;   // staging for the inputs (and a small single chunk's outputs)
    // dfmi_filter_project_host_batches' device region: two halves of
    // [headers (right-aligned in hcap) | outputs (ocap)], used alternately,
    // then the inputs + batch table (icap). A call's kernel zeroes the
    // headers the previous call left in the other half (hb_dirty: bytes at
    // the end of a half's header room that are not known to be zero).
    DevBuf hb;
    size_t hb_hcap = 0, hb_ocap = 0, hb_icap = 0, hb_dirty[2] = {0, 0};
    int hb_half = 0;
    HostBuf<uint8_t> hdr_pin;  // headers of the caller-owned form (dfmi_filter_project_host_batches_into)
    std::unique_ptr<host::Pool> pool;
    std::shared_ptr<host::PinnedPool> results = std::make_shared<host::PinnedPool>();

    Arena() {
        try {
            HIP_TRY(hipStreamCreateWithFlags(&h2d, hipStreamNonBlocking));
            HIP_TRY(hipStreamCreateWithFlags(&d2h, hipStreamNonBlocking));
            for (int s = 0; s < kSlots; ++s) {
                HIP_TRY(hipEventCreateWithFlags(&h2d_done[s], hipEventDisableTiming));
                HIP_TRY(hipEventCreateWithFlags(&d2h_done[s], hipEventDisableTiming));
                HIP_TRY(hipEventCreateWithFlags(&kdone[s], hipEventDisableTiming));
            }
            pool.reset(new host::Pool(host::host_threads() - 1));
        } catch (...) {
            close();
            throw;
        }
    }
    Arena(const Arena&) = delete;
    Arena& operator=(const Arena&) = delete;
    // The copy streams are drained before anything they use goes (the
    // buffers, pool and results are members: released after this body).
    ~Arena() { close(); }

    void reserve_hb(size_t H, size_t OB, size_t IM, hipStream_t st) {
        if (hb.p && H <= hb_hcap && OB <= hb_ocap && IM <= hb_icap) return;
        if (hb.p) HIP_TRY(hipStreamSynchronize(st));  // (earlier calls synchronised: nothing uses it)
        hb_hcap = std::max(H, std::max(hb_hcap, (size_t)64 << 10));
        hb_ocap = std::max(OB, hb_ocap);
        hb_icap = std::max(IM, hb_icap);
        hb.alloc(2 * (hb_hcap + hb_ocap) + hb_icap);
        for (int h = 0; h < 2; ++h) HIP_TRY(hipMemsetAsync(hb_half_base(h), 0, hb_hcap, st));
        hb_dirty[0] = hb_dirty[1] = 0;
    }
    uint8_t* hb_half_base(int h) const { return hb.as<uint8_t>() + (size_t)h * (hb_hcap + hb_ocap); }
    uint8_t* hb_inputs() const { return hb.as<uint8_t>() + 2 * (hb_hcap + hb_ocap); }

   private:
    void close() {
        if (h2d) (void)hipStreamSynchronize(h2d);
        if (d2h) (void)hipStreamSynchronize(d2h);
        for (int s = 0; s < kSlots; ++s) {
            if (h2d_done[s]) (void)hipEventDestroy(h2d_done[s]);
            if (d2h_done[s]) (void)hipEventDestroy(d2h_done[s]);
            if (kdone[s]) (void)hipEventDestroy(kdone[s]);
        }
        if (h2d) (void)hipStreamDestroy(h2d);
        if (d2h) (void)hipStreamDestroy(d2h);
        h2d = d2h = nullptr;
    }
};

// The context's arena, made on first use (the context's device is current).
inline Arena& arena_of(dfmi_context* ctx) {
    if (!ctx->host_arena) ctx->host_arena = new Arena();
    return *ctx->host_arena;
}

}  // namespace dfmi
