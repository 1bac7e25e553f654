// dfmi_generate_column (include/dfmi_datasource.h): host side of the
// datasource generator kernels (kernels.hip).
#include <hip/hip_runtime.h>

#include "../../include/dfmi_datasource.h"
#include "exec_internal.h"

using namespace dfmi;
using namespace dfmi::xi;

namespace dfmi {
hipError_t launch_gen_unit_f64(unsigned long long key, long long row0, long long n, double* out,
                               hipStream_t st);
hipError_t launch_gen_i64(unsigned long long key, long long row0, long long n, long long lo,
                          unsigned long long range, long long* out, hipStream_t st);
}  // namespace dfmi

static uint64_t host_splitmix64(uint64_t x) {
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

extern "C" int32_t dfmi_generate_column(dfmi_context* ctx, int32_t kind, uint64_t seed, uint32_t col,
                                        int64_t row0, int64_t n, int64_t lo, int64_t hi, void* out,
                                        dfmi_error* err) {
    return guarded(err, [&]() -> int32_t {
        if (!ctx || !out || n < 0) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "bad argument"};
        HIP_TRY(hipSetDevice(ctx->device));
        const uint64_t key = host_splitmix64(seed + (uint64_t)col * 0xD1B54A32D192ED03ull);
        if (kind == DFMI_GEN_UNIT_F64) {
            HIP_TRY(launch_gen_unit_f64(key, row0, n, (double*)out, ctx->stream));
        } else if (kind == DFMI_GEN_I64) {
            if (hi <= lo) throw Fail{DFMI_ERR_INVALID_ARGUMENT, "empty range"};
            HIP_TRY(launch_gen_i64(key, row0, n, lo, (uint64_t)(hi - lo), (long long*)out, ctx->stream));
        } else {
            throw Fail{DFMI_ERR_INVALID_ARGUMENT, "unknown generator"};
        }
        return DFMI_OK;
    });
}
