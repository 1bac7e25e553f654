// dfmi_context: its lifecycle, settings and what the last call left in it
// (timings, the error's evaluation-order key, the kernel's name), and the
// ABI version.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <new>

#include "exec_internal.h"

using namespace dfmi;
using namespace dfmi::xi;

extern "C" int32_t dfmi_context_create(int32_t device, void* stream, dfmi_context** out, dfmi_error* err) {
    set_err(err, DFMI_OK, "");
    if (!out) {
        set_err(err, DFMI_ERR_INVALID_ARGUMENT, "out is NULL");
        return DFMI_ERR_INVALID_ARGUMENT;
    }
    dfmi_context* c = new (std::nothrow) dfmi_context();
    if (!c) return DFMI_ERR_INVALID_ARGUMENT;
    return guarded(err, [&]() -> int32_t {
        HIP_TRY(hipSetDevice(device));
        c->device = device;
        c->stream = (hipStream_t)stream;
        if (const char* e = getenv("DFMI_SHARED")) c->shared = atoi(e) != 0;
        c->host_hdr.resize(kHdrAlloc, dfmi::kGrowExact);

        HIP_TRY(hipEventCreate(&c->ev0));
        HIP_TRY(hipEventCreate(&c->ev1));
        HIP_TRY(hipEventCreate(&c->ev2));
        *out = c;
        return DFMI_OK;
    }, [&] {
        delete c;
    });
}

namespace dfmi {
void sort_scratch_release(dfmi_context* c);
void format_scratch_release(dfmi_context* c);
void csv_scratch_release(dfmi_context* c);
}  // namespace dfmi

extern "C" void dfmi_context_destroy(dfmi_context* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    dfmi::host_arena_release(c);
    dfmi::sort_scratch_release(c);
    dfmi::format_scratch_release(c);
    dfmi::csv_scratch_release(c);
    if (c->ev0) (void)hipEventDestroy(c->ev0);
    if (c->ev1) (void)hipEventDestroy(c->ev1);
    if (c->ev2) (void)hipEventDestroy(c->ev2);
    delete c;
}

extern "C" int32_t dfmi_context_set_stream(dfmi_context* c, void* stream) {
    if (!c) return DFMI_ERR_INVALID_ARGUMENT;
    c->stream = (hipStream_t)stream;
    return DFMI_OK;
}

extern "C" int32_t dfmi_abi_version(void) { return DFMI_ABI_VERSION; }

extern "C" int32_t dfmi_context_set_shared(dfmi_context* c, int32_t shared) {
    if (!c) return DFMI_ERR_INVALID_ARGUMENT;
    c->shared = shared != 0;
    return DFMI_OK;
}

extern "C" int32_t dfmi_context_set_timing(dfmi_context* c, int32_t enable) {
    if (!c) return DFMI_ERR_INVALID_ARGUMENT;
    c->timing = enable != 0;
    return DFMI_OK;
}

extern "C" int32_t dfmi_last_timing(const dfmi_context* c, double* total_ms, double* main_ms) {
    if (!c || !c->timed) return DFMI_ERR_INVALID_ARGUMENT;
    if (total_ms) *total_ms = c->last_total_ms;
    if (main_ms) *main_ms = c->last_main_ms;
    return DFMI_OK;
}

extern "C" int32_t dfmi_last_error_order(const dfmi_context* c, uint64_t* key) {
    if (!c || !key) return DFMI_ERR_INVALID_ARGUMENT;
    *key = c->last_err_key;
    return DFMI_OK;
}

// Internal test hook: look-back timeouts relaunched on this context.
extern "C" long dfmi_internal_relaunches(const dfmi_context* c) { return c ? c->relaunches : -1; }
// Internal test hook: the hipRTC module cache's size after bounding it to
// `cap` modules (cap > 0; 0 leaves the bound unchanged).
extern "C" int64_t dfmi_internal_jit_cache(int64_t cap) {
    jit::cache_cap(cap > 0 ? (size_t)cap : 0);
    return (int64_t)jit::cache_size();
}

extern "C" const char* dfmi_last_kernel_name(const dfmi_context* c) {
    return c ? c->last_kernel.c_str() : "";
}

extern "C" int32_t dfmi_last_compile_ms(const dfmi_context* c, double* compile_ms) {
    if (!c || !compile_ms) return DFMI_ERR_INVALID_ARGUMENT;
    *compile_ms = c->last_compile_ms;
    return DFMI_OK;
}

