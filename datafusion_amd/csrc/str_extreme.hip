// MIN / MAX over a Utf8 argument: the fixed gfx950 kernels of the string side
// structure (str_extreme.h has the protocol and the visibility rule;
// agg_strext.cpp drives them). The order is the GROUP BY / ORDER BY /
// DFMI_FLAG_EXT_UTF8_ORDER one: sequences of unsigned bytes, the first
// differing byte decides, a proper prefix is less; the empty string is the
// least value.
#include <hip/hip_runtime.h>

#include "groupby.h"
#include "str_extreme.h"

namespace dfmi {
namespace sx {

typedef unsigned long long u64;
typedef unsigned char u8;

__device__ __forceinline__ bool counted(const Args& A, long long i) {
    return !A.validity || ((A.validity[i >> 3] >> (i & 7)) & 1);
}

// The first 8 bytes big-endian, zero-padded: word order = byte order up to 8 bytes.
__device__ __forceinline__ u64 prefix_of(const u8* p, unsigned len) {
    u64 v = 0;
#pragma unroll
    for (unsigned q = 0; q < 8; ++q) v = (v << 8) | (q < len ? (u64)p[q] : 0ull);
    return v;
}

// < 0, 0, > 0: a against b bytewise, a proper prefix less.
__device__ __forceinline__ int compare_bytes(const u8* a, unsigned la, const u8* b, unsigned lb) {
    const unsigned n = la < lb ? la : lb;
    for (unsigned q = 0; q < n; ++q)
        if (a[q] != b[q]) return a[q] < b[q] ? -1 : 1;
    return la == lb ? 0 : (la < lb ? -1 : 1);
}

__device__ __forceinline__ bool row_of(const Args& A, long long i, unsigned& g) {
    g = A.rg ? A.rg[i] : 0u;
    return g != kNone && (u64)g < A.ngroups && counted(A, i);
}

__global__ __launch_bounds__(256) void k_sx_init(u64* pref, unsigned* best, Ent* ent, int is_min, u64 g0, u64 g1) {
    for (u64 g = g0 + (u64)blockIdx.x * blockDim.x + threadIdx.x; g < g1; g += (u64)gridDim.x * blockDim.x) {
        pref[g] = is_min ? ~0ull : 0ull;
        best[g] = kNone;
        ent[g].off = 0;
        ent[g].len = kNone;
        ent[g].pad = 0;
    }
}

// Prefix pass, one group (ungrouped): a running extreme per thread over a
// grid-stride loop, reduced across the wave; one atomic per wave.
__global__ __launch_bounds__(256) void k_sx_prefix_one(const Args A) {
    const bool is_min = A.is_min != 0;
    u64 run = is_min ? ~0ull : 0ull;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < A.m; i += (long long)gridDim.x * blockDim.x) {
        if (!counted(A, i)) continue;
        const int a = A.offsets[i], b = A.offsets[i + 1];
        const u64 p = prefix_of(A.bytes + a, (unsigned)(b - a));
        run = is_min ? (p < run ? p : run) : (p > run ? p : run);
    }
    for (int d = 32; d >= 1; d >>= 1) {
        const u64 o = __shfl_xor(run, d, 64);
        run = is_min ? (o < run ? o : run) : (o > run ? o : run);
    }
    // (a wave without a counted row holds the identity, which pref starts from)
    if ((threadIdx.x & 63) == 0) {
        if (is_min) atomicMin(&A.pref[0], run);
        else atomicMax(&A.pref[0], run);
    }
}

// Prefix pass, grouped: a row adds only if its prefix beats a plain pre-read
// of the word (monotonic: a stale value is an older, no-better one).
__global__ __launch_bounds__(256) void k_sx_prefix(const Args A) {
    const bool is_min = A.is_min != 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < A.m; i += (long long)gridDim.x * blockDim.x) {
        unsigned g;
        if (!row_of(A, i, g)) continue;
        const int a = A.offsets[i], b = A.offsets[i + 1];
        const u64 p = prefix_of(A.bytes + a, (unsigned)(b - a));
        const u64 seen = A.pref[g];
        if (is_min ? p < seen : p > seen) {
            if (is_min) atomicMin(&A.pref[g], p);
            else atomicMax(&A.pref[g], p);
        }
    }
}

// Row i against what `cur` names: a batch row, or the persisted winner.
__device__ __forceinline__ bool beats(const Args& A, const u8* s, unsigned len, unsigned g, unsigned cur) {
    const u8* o;
    unsigned olen;
    if (cur == kNone) {
        const Ent e = A.ent[g];
        if (e.len == kNone) return true;  // no value yet
        o = A.arena + e.off;
        olen = e.len;
    } else {
        const int a = A.offsets[cur], b = A.offsets[cur + 1];
        o = A.bytes + a;
        olen = (unsigned)(b - a);
    }
    const int c = compare_bytes(s, len, o, olen);
    return A.is_min ? c < 0 : c > 0;
}

// Candidate pass (a launch after the prefix pass: pref is final for the batch).
__global__ __launch_bounds__(256) void k_sx_candidates(const Args A) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < A.m; i += (long long)gridDim.x * blockDim.x) {
        unsigned g;
        if (!row_of(A, i, g)) continue;
        const int a = A.offsets[i], b = A.offsets[i + 1];
        const u8* s = A.bytes + a;
        const unsigned len = (unsigned)(b - a);
        if (prefix_of(s, len) != A.pref[g]) continue;
        unsigned cur = A.best[g];  // plain: a stale value is an older, no-better winner
        while (beats(A, s, len, g, cur)) {
            const unsigned old = atomicCAS(&A.best[g], cur, (unsigned)i);
            if (old == cur) break;
            cur = old;  // another row won meanwhile: against that one
        }
    }
}

// Measure pass (best is final): the bytes the keep pass will reserve, one atomic per wave.
__global__ __launch_bounds__(256) void k_sx_measure(const Args A) {
    u64 sum = 0;
    for (u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x; g < A.ngroups; g += (u64)gridDim.x * blockDim.x) {
        const unsigned r = A.best[g];
        if (r == kNone || (long long)r >= A.m) continue;
        sum += (u64)(unsigned)(A.offsets[r + 1] - A.offsets[r]);
    }
    for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d, 64);
    if ((threadIdx.x & 63) == 0 && sum) atomicAdd(&A.hdr->need, sum);
}

// Keep pass: the batch's winners persisted (a launch of its own: best is final).
__global__ __launch_bounds__(256) void k_sx_keep(const Args A) {
    for (u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x; g < A.ngroups; g += (u64)gridDim.x * blockDim.x) {
        const unsigned r = A.best[g];
        if (r == kNone) continue;
        A.best[g] = kNone;
        if ((long long)r >= A.m) continue;
        const int a = A.offsets[r], b = A.offsets[r + 1];
        const unsigned len = (unsigned)(b - a);
        const u64 off = atomicAdd(&A.hdr->arena_end, (u64)len);
        if (off + len > A.arena_cap) continue;  // (the host reserved the batch's bytes: it checks arena_end)
        for (unsigned q = 0; q < len; ++q) A.arena[off + q] = A.bytes[a + q];
        const unsigned was = A.ent[g].len;  // the superseded winner's bytes are garbage from here on
        atomicAdd(&A.hdr->live, (u64)len - (u64)(was == kNone ? 0u : was));  // (modulo 2^64: a signed step)
        Ent e;
        e.off = off;
        e.len = len;
        e.pad = 0;
        A.ent[g] = e;
    }
}

__global__ __launch_bounds__(256) void k_sx_compact(Ent* ent, u64 ngroups, const u8* from, u8* to, u64 to_cap, Hdr* to_hdr) {
    for (u64 g = (u64)blockIdx.x * blockDim.x + threadIdx.x; g < ngroups; g += (u64)gridDim.x * blockDim.x) {
        const Ent e = ent[g];
        if (e.len == kNone) continue;
        const u64 off = atomicAdd(&to_hdr->arena_end, (u64)e.len);
        if (off + e.len > to_cap) continue;
        for (unsigned q = 0; q < e.len; ++q) to[off + q] = from[e.off + q];
        ent[g].off = off;
    }
}

// Workgroups for `items`, at most `cap` -- at most `diag` when that is set
// (DFMI_GROUP_GRID, groupby.h "Diagnostic grid cap"); a launch that needs more
// than one trip of its grid counts itself.
static int grid_for(long long items, int diag, int cap = 1024) {
    if (diag > 0 && diag < cap) cap = diag;
    const long long g = (items + 255) / 256;
    const int blocks = (int)(g < 1 ? 1 : (g > cap ? cap : g));
    if (items > (long long)blocks * 256) gb::count_strided_launch();
    return blocks;
}

hipError_t launch_init(u64* pref, unsigned* best, Ent* ent, int is_min, u64 g0, u64 g1, int grid, hipStream_t st) {
    if (g1 <= g0) return hipSuccess;
    hipLaunchKernelGGL(k_sx_init, dim3(grid_for((long long)(g1 - g0), grid)), dim3(256), 0, st, pref, best, ent, is_min, g0,
                       g1);
    return hipGetLastError();
}

hipError_t launch_find(const Args& a, int grid, hipStream_t st) {
    if (a.m <= 0 || !a.ngroups) return hipSuccess;
    // one group: a few thousand atomics on its one word per batch (one per wave of a capped grid)
    if (!a.rg) hipLaunchKernelGGL(k_sx_prefix_one, dim3(grid_for(a.m, grid, 512)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(k_sx_prefix, dim3(grid_for(a.m, grid)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_sx_candidates, dim3(grid_for(a.m, grid)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_sx_measure, dim3(grid_for((long long)a.ngroups, grid)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_keep(const Args& a, int grid, hipStream_t st) {
    if (a.m <= 0 || !a.ngroups) return hipSuccess;
    hipLaunchKernelGGL(k_sx_keep, dim3(grid_for((long long)a.ngroups, grid)), dim3(256), 0, st, a);
    return hipGetLastError();
}

hipError_t launch_compact(Ent* ent, u64 ngroups, const u8* from, u8* to, u64 to_cap, Hdr* to_hdr, int grid,
                          hipStream_t st) {
    if (!ngroups) return hipSuccess;
    hipLaunchKernelGGL(k_sx_compact, dim3(grid_for((long long)ngroups, grid)), dim3(256), 0, st, ent, ngroups, from, to,
                       to_cap, to_hdr);
    return hipGetLastError();
}

}  // namespace sx
}  // namespace dfmi
