// MIN / MAX over a Utf8 argument (DFMI_FLAG_EXT_AGG_MINMAX_ANY): the side
// structure that keeps, per Utf8 extreme and dense group id (one group when
// ungrouped), the extreme string seen so far. Inside the record machinery
// such an aggregate is a COUNT (agg_host.h acc_fn); the strings live here.
//
// Per extreme and group:
//   pref  u64: the extreme of the counted rows' first 8 bytes, packed
//         big-endian and zero-padded (so the word order is the byte order up
//         to 8 bytes; "a" and "a\0" share a word and the candidate pass
//         decides);
//   ent   the persisted winner: (arena offset, length), length kNone: none;
//   best  u32: the batch row that beats the persisted winner so far, or
//         kNone: "the persisted one".
// Per batch, after the rows' groups are known, these launches:
//   prefix      every counted row folds its prefix into pref[g] (64-bit
//               atomic min / max; a row whose prefix does not beat a plain
//               pre-read of the word -- a stale value is an older, no-better
//               one -- issues no atomic; ungrouped: a running extreme per
//               thread, one atomic per wave);
//   candidates  a row whose prefix equals pref[g] runs an arg-extreme
//               compare-and-swap loop on best[g] with the full bytewise
//               comparator, against the batch row or the persisted bytes the
//               current value names (pre-read plain, as above);
//   measure     the bytes of the rows that best names, summed into
//               Hdr::need: what the keep pass will reserve, so the host makes
//               exactly that much room (not the whole argument column's);
//   keep        a group whose best names a batch row reserves arena bytes
//               (atomic add on Hdr::arena_end), copies the row's bytes,
//               stores (offset, length), resets best and keeps Hdr::live.
// Visibility (per-XCD L2s are not coherent within a launch): the only words
// both written and read by one launch are pref / best, through atomics (and
// the monotonic pre-read); string bytes and persisted entries a launch reads
// were written by an earlier launch or are the batch's read-only input.
// The host guarantees arena room for the measured bytes before keep;
// superseded strings are dropped by compacting into a fresh arena.
#ifndef DFMI_STR_EXTREME_H
#define DFMI_STR_EXTREME_H

#include <hip/hip_runtime.h>

#include <cstdint>

namespace dfmi {
namespace sx {

constexpr unsigned kNone = 0xffffffffu;

struct Ent {
    unsigned long long off;  // arena offset
    unsigned len;            // bytes; kNone: no value yet
    unsigned pad;
};

struct Hdr {
    unsigned long long arena_end;  // bytes reserved
    unsigned long long need;       // the measure pass: bytes the batch's keep passes will reserve
    unsigned long long live;       // bytes of the persisted winners (reserved less superseded)
};

// One Utf8 extreme's state over `ngroups` groups and one batch's argument column.
struct Args {
    const unsigned char* bytes;   // the evaluated argument column: Utf8 bytes,
    const int32_t* offsets;       // offsets (m + 1),
    const unsigned char* validity;  // validity (nullptr: every row counts)
    const unsigned* rg;           // the row's dense group id (~0u: not added on the device); nullptr: group 0
    long long m;                  // rows
    int is_min;
    unsigned long long ngroups;
    unsigned long long* pref;
    unsigned* best;
    Ent* ent;
    unsigned char* arena;
    unsigned long long arena_cap;
    Hdr* hdr;
};

// launches on `stream` (asynchronous); grid: groupby.h "Diagnostic grid cap" (0: the launch's own cap)
hipError_t launch_init(unsigned long long* pref, unsigned* best, Ent* ent, int is_min, unsigned long long g0,
                       unsigned long long g1, int grid, hipStream_t stream);
hipError_t launch_find(const Args& a, int grid, hipStream_t stream);  // prefix, candidates, measure (adds to Hdr::need)
hipError_t launch_keep(const Args& a, int grid, hipStream_t stream);
// every live string of `ent` copied from `from` into `to` (reserving at to_hdr), ent[g].off updated
hipError_t launch_compact(Ent* ent, unsigned long long ngroups, const unsigned char* from, unsigned char* to,
                          unsigned long long to_cap, Hdr* to_hdr, int grid, hipStream_t stream);

}  // namespace sx
}  // namespace dfmi

#endif
