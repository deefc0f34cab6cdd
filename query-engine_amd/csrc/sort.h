// What the radix sort (k_sort.hip) exports to the other units: the permutation sort and its passes
// (k_window_sort.hip, k_partition.hip), the payload sort (k_merge.hip, executor.hip) and the pieces
// the top-k select builds on (k_topk.hip).
#pragma once
#include <algorithm>

#include "ops.h"

namespace qeh {

// Sort state: encoded keys + permutation, double-buffered.
struct RadixState {
    DevBuf k[2], v[2];
    int cur = 0;
    int64_t n = 0;
    bool enc_injective = false;  // k[cur] encodes the last-sorted column one-to-one (no null-flag pass)
    int part_shift = -1;         // >= 0: k[cur] holds (first key << part_shift) | ..., the pair encoding
    bool key32 = false;          // k[] currently holds 32-bit keys (column range fits 32 bits)
};

// ballot ranking when asked for (QEH_RS_BALLOT=1, A/B) or when the device's LDS atomics failed the
// lane-order self-check (lds_atomic_rank_ok)
inline bool rs_ballot(qeh_ctx *ctx) {
    return std::getenv("QEH_RS_BALLOT") != nullptr || !lds_atomic_rank_ok(ctx);
}

inline int gc_of(qeh_ctx *ctx, int64_t nchunks) {
    return (int)std::min<int64_t>(nchunks, (int64_t)ctx->props.multiProcessorCount * 8);
}

inline int bit_length(uint64_t x) {
    int b = 0;
    while (b < 64 && (x >> b) != 0) ++b;
    return b;
}

// Stable LSD passes over the low `bits` of the encoded keys in rs (u32 / u64 as rs.key32 says).
int radix_passes(qeh_ctx *ctx, RadixState &rs, int bits);
// One stable pass on the 8-bit digit at `shift`.
int radix_pass_at(qeh_ctx *ctx, RadixState &rs, int shift);
// The per-segment histogram of a byte stream (k_rs_hist_u8): block b counts ids[b * seg, (b + 1) * seg)
// into hist[digit * nblocks + b].  Launch only; the caller checks hipGetLastError.
void launch_hist_u8(qeh_ctx *ctx, const uint8_t *ids, int64_t n, int64_t seg, uint32_t *hist, int nblocks);

// qeh_sort_indices' key checks: at least one key, equal lengths (*n), no Utf8 left.
int check_sort_keys(const qeh_column *keys, int n_keys, int64_t *n);
// Stable lexicographic permutation by keys (last key sorted first) into rs.v[rs.cur].
int sort_perm(qeh_ctx *ctx, const qeh_column *keys, int n_keys, const int8_t *ascending, int64_t n, RadixState &rs,
              const int8_t *nulls_first = nullptr);

// Stable sort of (one Int64 / Int32 key, one non-null 8-byte payload) carrying the payload through
// the radix passes (no gather): the sorted key and payload columns.  kPayloadSortNotEligible when
// the shapes do not fit (nothing allocated).
constexpr int kPayloadSortNotEligible = -3;
int sort_pairs_payload_parts(qeh_ctx *ctx, const qeh_column *keys, const qeh_column *vals, int nparts, bool asc,
                             bool nulls_first, qeh_column *out_key, qeh_column *out_val);
int sort_pairs_payload(qeh_ctx *ctx, const qeh_column &key, const qeh_column &val, bool asc, bool nulls_first,
                       qeh_column *out_key, qeh_column *out_val);
// For the top-k select: min / max of a key column's ordered values over its non-NULL rows (mn > mx:
// none; one synchronous read); and the first min(limit, n) entries of the stable sort permutation of
// `keys` as a fresh UINT32 column, mapped through rows[] when given (the keys are then those of rows
// rows[0..n)).
int sort_key_range(qeh_ctx *ctx, const qeh_column &col, int64_t *mn, int64_t *mx);
int sort_perm_prefix(qeh_ctx *ctx, const qeh_column *keys, int n_keys, const int8_t *ascending, int64_t n, int64_t limit,
                     const uint32_t *rows, qeh_column *out_perm);

}  // namespace qeh
