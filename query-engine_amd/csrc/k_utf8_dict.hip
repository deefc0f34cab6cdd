// Order-preserving dictionary encoding of a Utf8 column (qeh_utf8_dict_encode) and the helper that
// lets Utf8 columns be GROUP BY / ORDER BY / PARTITION BY keys: every Utf8 key is replaced by its
// INT32 code column, whose integer order is the strings' byte-wise (unsigned) lexicographic order --
// arrow's order on StringArray, the order k_utf8_cmp uses.
//
//  (a) distinct pass (streams the n rows once): each lane hashes its row's bytes to 64 bits and
//      probes a global open-addressing table of 64-bit words (hash tag << 32 | representative
//      row + 1; 0 = empty).  An empty word is claimed with one atomicCAS; on an equal tag the
//      lane compares its bytes with the representative row's and adopts the slot or probes on.
//      A per-workgroup LDS table of recently resolved (tag -> slot) hints is tried first, so a
//      column of few distinct strings costs no global atomic read-modify-write per row.  A probe
//      gives up after kMaxProbe steps, and a table more than half full stops taking rows: both
//      set the overflow word and the host retries with a larger table (16x once, then 2n slots,
//      which n rows cannot half fill).  Claimed slots are counted once per wave.
//  (b) the occupied slots are compacted into D representative rows (scan of the occupancy).
//  (c) the D representatives are ordered in host-driven rounds r = 0, 1, ...: bytes [8r, 8r+8)
//      of every representative packed big-endian into one word (zero past the end) plus the
//      remaining length clamped to 0..8, sorted by (segment, word, remaining length) with the
//      radix sort of k_sort.hip, segments split where the triple differs.  The remaining length
//      puts a string before any longer one that only adds 0x00 bytes.  Cost ~ D per round.
//  (d) rank[slot], then codes[i] = rank[slot_of_row[i]] in one streaming pass; the dictionary is
//      gather_column over the sorted representatives.
//
// Join keys (qeh_utf8_join_encode) need equality only and one dictionary for two columns: (a) and
// the occupancy scan of (b) run over the build column, whose codes are dense[slot_of_row[i]] -- dense
// in [0, D) but unordered, (c) is skipped -- and k_dict_lookup streams the probe column once against
// the finished table: a probe string found there takes the build string's code, any other row is NULL.
//
// All traffic between workgroups inside one launch goes through atomic words of the table and the
// control words; the only bytes a lane compares against are the input column's, which no launch
// writes.  Every kernel loop is bounded; no lane waits on another.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "device_common.h"
#include "ops.h"

namespace qeh {

constexpr int kDictMaxProbe = 4096;   // probe steps before a row reports overflow
constexpr int kDictHintLog2 = 10;     // LDS hints per workgroup (8 KiB)
constexpr int kDictDefaultCapLog2 = 14;
constexpr int kDictMaxCapLog2 = 31;   // slot + 1 fits 32 bits; D <= INT32_MAX anyway

struct DictIn {
    ColRef valid;          // validity only
    const int32_t *offs;   // advanced by the column offset
    const uint8_t *data;
};

// control words of the distinct pass
enum { DC_OVERFLOW = 0, DC_COUNT = 1, DC_MAXLEN = 2, DC_WORDS = 4 };

// up to 8 bytes at p as a little-endian word; only p[0 .. min(rem, 8)) is read
__device__ __forceinline__ uint64_t load8(const uint8_t *p, int32_t rem) {
    uint64_t w = 0;
    if (rem >= 8) {
        __builtin_memcpy(&w, p, 8);
    } else {
#pragma unroll
        for (int b = 0; b < 7; ++b)
            if (b < rem) w |= (uint64_t)p[b] << (8 * b);
    }
    return w;
}

__device__ __forceinline__ uint64_t str_hash(const uint8_t *p, int32_t len) {
    uint64_t h = 0x9E3779B97F4A7C15ull ^ (uint64_t)(uint32_t)len;
    for (int32_t o = 0; o < len; o += 8) {
        h = (h ^ load8(p + o, len - o)) * 0xFF51AFD7ED558CCDull;
        h ^= h >> 32;
    }
    h *= 0xC4CEB9FE1A85EC53ull;
    return h ^ (h >> 29);
}

__device__ __forceinline__ bool str_eq(const uint8_t *a, const uint8_t *b, int32_t len) {
    for (int32_t o = 0; o < len; o += 8)
        if (load8(a + o, len - o) != load8(b + o, len - o)) return false;
    return true;
}

__device__ __forceinline__ uint64_t ld_relaxed(const uint64_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t ld_relaxed(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// (a) slot_of_row[i] = the table slot holding row i's string (valid rows; NULL rows get 0, unused)
__global__ __launch_bounds__(kBlock) void k_dict_insert(DictIn in, int64_t n, uint64_t *__restrict__ table, int cap_log2,
                                                        uint64_t hash_mask, uint32_t count_limit,
                                                        uint32_t *__restrict__ slot_of_row, uint32_t *__restrict__ ctl) {
    __shared__ uint64_t hint[1 << kDictHintLog2];  // tag << 32 | slot + 1; a stale or torn hint is only a miss
    for (int t = threadIdx.x; t < (1 << kDictHintLog2); t += kBlock) hint[t] = 0;
    __syncthreads();
    const uint32_t cap_mask = (uint32_t)((1ull << cap_log2) - 1ull);
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        if (ld_relaxed(&ctl[DC_OVERFLOW])) return;  // the host retries with a larger table
        if (!col_valid(in.valid, i)) {
            slot_of_row[i] = 0;
            continue;
        }
        const int32_t s = in.offs[i], len = in.offs[i + 1] - s;
        const uint8_t *p = in.data + s;
        const uint64_t h = str_hash(p, len) & hash_mask;
        const uint32_t tag = (uint32_t)(h >> 32);
        const uint32_t hi = (uint32_t)((h * 0xD6E8FEB86659FD93ull) >> (64 - kDictHintLog2));
        const uint64_t hv = hint[hi];
        if (hv != 0 && (uint32_t)(hv >> 32) == tag) {
            const uint32_t slot = ((uint32_t)hv - 1u) & cap_mask;
            const uint64_t w = ld_relaxed(&table[slot]);
            if (w != 0 && (uint32_t)(w >> 32) == tag) {
                const int64_t r = (int64_t)(uint32_t)w - 1;
                const int32_t rs = in.offs[r];
                if (in.offs[r + 1] - rs == len && str_eq(p, in.data + rs, len)) {
                    slot_of_row[i] = slot;
                    continue;
                }
            }
        }
        uint32_t idx = (uint32_t)((h * 0x9E3779B97F4A7C15ull) >> (64 - cap_log2));
        const uint64_t mine = ((uint64_t)tag << 32) | (uint64_t)(uint32_t)(i + 1);
        bool resolved = false, claimed = false;
        for (int step = 0; step < kDictMaxProbe; ++step) {
            uint64_t w = ld_relaxed(&table[idx]);
            if (w == 0) {
                const uint64_t prev = atomicCAS((unsigned long long *)&table[idx], 0ull, (unsigned long long)mine);
                if (prev == 0) {
                    resolved = claimed = true;
                    break;
                }
                w = prev;
            }
            if ((uint32_t)(w >> 32) == tag) {
                const int64_t r = (int64_t)(uint32_t)w - 1;
                const int32_t rs = in.offs[r];
                if (in.offs[r + 1] - rs == len && str_eq(p, in.data + rs, len)) {
                    resolved = true;
                    break;
                }
            }
            idx = (idx + 1u) & cap_mask;
        }
        // one counter update per wave, not per claimed slot (all-distinct columns claim every row)
        const uint64_t here = __ballot(1), won = __ballot(claimed);
        if (won != 0 && (threadIdx.x & 63) == (unsigned)(__ffsll((unsigned long long)here) - 1)) {
            const uint32_t c = (uint32_t)__popcll(won);
            if (atomicAdd(&ctl[DC_COUNT], c) + c > count_limit) atomicOr(&ctl[DC_OVERFLOW], 1u);
        }
        if (resolved) hint[hi] = ((uint64_t)tag << 32) | (uint64_t)(idx + 1u);
        else atomicOr(&ctl[DC_OVERFLOW], 1u);
        slot_of_row[i] = resolved ? idx : 0u;
    }
}

// (b) occupancy of the table (scanned into dense ids), then the representative row of each dense id
__global__ void k_dict_occupied(const uint64_t *__restrict__ table, uint64_t cap, uint32_t *__restrict__ occ) {
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += (uint64_t)gridDim.x * blockDim.x)
        occ[s] = table[s] != 0 ? 1u : 0u;
}

__global__ void k_dict_reps(const uint64_t *__restrict__ table, uint64_t cap, const uint64_t *__restrict__ dense,
                            uint32_t *__restrict__ rep_row) {
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t w = table[s];
        if (w != 0) rep_row[dense[s]] = (uint32_t)w - 1u;
    }
}

// (c) round r: bytes [8r, 8r+8) of every representative, big-endian with the sign bit flipped (so
// the Int64 sort orders them as unsigned words), and the remaining length clamped to 0..8
__global__ __launch_bounds__(kBlock) void k_dict_pack(DictIn in, const uint32_t *__restrict__ rep_row, int64_t d, int32_t byte0,
                                                      int64_t *__restrict__ word, int32_t *__restrict__ rem,
                                                      uint32_t *__restrict__ ctl) {
    for (int64_t base = (int64_t)blockIdx.x * kBlock; base < d; base += (int64_t)gridDim.x * kBlock) {
        const int64_t j = base + threadIdx.x;
        int32_t len = 0;
        if (j < d) {
            const int64_t r = rep_row[j];
            const int32_t s = in.offs[r];
            len = in.offs[r + 1] - s;
            const int32_t left = len > byte0 ? len - byte0 : 0;
            const uint64_t w = left > 0 ? __builtin_bswap64(load8(in.data + s + byte0, left)) : 0ull;
            word[j] = (int64_t)(w ^ 0x8000000000000000ull);
            rem[j] = left < 8 ? left : 8;
        }
        if (ctl) {  // the longest representative bounds the number of rounds
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) {
                const int32_t x = __shfl_xor(len, o, 64);
                len = x > len ? x : len;
            }
            if ((threadIdx.x & 63) == 0 && len > 0) atomicMax(&ctl[DC_MAXLEN], (uint32_t)len);
        }
    }
}

// sorted position i starts a new segment when its (segment, word, remaining length) differs from i-1's
__global__ void k_dict_flags(const uint32_t *__restrict__ perm, const int32_t *__restrict__ seg, const int64_t *__restrict__ word,
                             const int32_t *__restrict__ rem, int64_t d, uint32_t *__restrict__ flags) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d; i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t f = 1;
        if (i > 0) {
            const uint32_t a = perm[i - 1], b = perm[i];
            f = (seg && seg[a] != seg[b]) || word[a] != word[b] || rem[a] != rem[b];
        }
        flags[i] = f;
    }
}

__global__ void k_dict_segments(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ flags,
                                const uint64_t *__restrict__ excl, int64_t d, int32_t *__restrict__ seg) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d; i += (int64_t)gridDim.x * blockDim.x)
        seg[perm[i]] = (int32_t)(excl[i] + flags[i] - 1);
}

// the order found: sorted_row[i] = the i-th smallest string's representative row, rank_of_rep its inverse
__global__ void k_dict_ranks(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ rep_row, int64_t d,
                             uint32_t *__restrict__ sorted_row, uint32_t *__restrict__ rank_of_rep) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < d; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t j = perm[i];
        sorted_row[i] = rep_row[j];
        rank_of_rep[j] = (uint32_t)i;
    }
}

// (d) rank of every occupied slot, then the codes
__global__ void k_dict_slot_ranks(const uint64_t *__restrict__ table, uint64_t cap, const uint64_t *__restrict__ dense,
                                  const uint32_t *__restrict__ rank_of_rep, uint32_t *__restrict__ rank_of_slot) {
    for (uint64_t s = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; s < cap; s += (uint64_t)gridDim.x * blockDim.x)
        rank_of_slot[s] = table[s] != 0 ? rank_of_rep[dense[s]] : 0u;
}

// (R = uint32_t: the ranks of (c); R = uint64_t: the scan's dense ids, the unordered join codes)
template <typename R>
__global__ void k_dict_codes(ColRef valid, const uint32_t *__restrict__ slot_of_row, const R *__restrict__ rank_of_slot,
                             int64_t n, int32_t *__restrict__ codes, uint64_t *__restrict__ out_valid) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * (blockDim.x / 64);
    for (int64_t w = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); w * 64 < n; w += nw) {
        const int64_t i = w * 64 + lane;
        const bool v = i < n && col_valid(valid, i);
        if (i < n) codes[i] = v ? (int32_t)rank_of_slot[slot_of_row[i]] : 0;
        const uint64_t vb = __ballot(v);
        if (lane == 0 && out_valid) out_valid[w] = vb;
    }
}

// Join probe side: the code of every probe row whose string the finished table of the build column
// holds; every other row (NULL, or a string the build side lacks) gets 0 and a cleared validity bit.
// The table is read-only here (a launch of its own after the insert loop has ended): plain loads, no
// atomics, no writes.  Same hash, mask and home slot as k_dict_insert.  The walk stops at an empty
// word or after kDictMaxProbe steps: k_dict_insert placed every stored string within kDictMaxProbe
// steps of its home slot over words that were all occupied by then, and no slot is ever vacated, so
// a string not met on the way to the first empty word, or within the bound, is not in the table.
// No per-workgroup LDS hint table as in k_dict_insert: with 1e6 build strings it was no faster
// (14.37 ms against 14.24 ms per 1e8 probe rows, DESIGN.md §5 "Utf8 join keys").
__global__ __launch_bounds__(kBlock) void k_dict_lookup(DictIn probe, int64_t n, DictIn build,
                                                        const uint64_t *__restrict__ table, int cap_log2, uint64_t hash_mask,
                                                        const uint64_t *__restrict__ dense, int32_t *__restrict__ codes,
                                                        uint64_t *__restrict__ out_valid) {
    const int lane = threadIdx.x & 63;
    const uint32_t cap_mask = (uint32_t)((1ull << cap_log2) - 1ull);
    const int64_t nw = (int64_t)gridDim.x * (kBlock / 64);
    for (int64_t w = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); w * 64 < n; w += nw) {
        const int64_t i = w * 64 + lane;
        bool found = false;
        int32_t code = 0;
        if (i < n && col_valid(probe.valid, i)) {
            const int32_t s = probe.offs[i], len = probe.offs[i + 1] - s;
            const uint8_t *p = probe.data + s;
            const uint64_t h = str_hash(p, len) & hash_mask;
            const uint32_t tag = (uint32_t)(h >> 32);
            uint32_t idx = (uint32_t)((h * 0x9E3779B97F4A7C15ull) >> (64 - cap_log2));
            for (int step = 0; step < kDictMaxProbe; ++step) {
                const uint64_t t = table[idx];
                if (t == 0) break;
                if ((uint32_t)(t >> 32) == tag) {
                    const int64_t r = (int64_t)(uint32_t)t - 1;
                    const int32_t rs = build.offs[r];
                    if (build.offs[r + 1] - rs == len && str_eq(p, build.data + rs, len)) {
                        found = true;
                        code = (int32_t)dense[idx];
                        break;
                    }
                }
                idx = (idx + 1u) & cap_mask;
            }
        }
        if (i < n) codes[i] = code;
        const uint64_t vb = __ballot(found);
        if (lane == 0) out_valid[w] = vb;
    }
}

// codes of an aggregate's output key column -> gather indices into the dictionary (NULL -> kNullRow)
__global__ void k_dict_code_idx(ColRef codes, int64_t n, uint32_t *__restrict__ idx) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        idx[i] = col_valid(codes, i) ? (uint32_t)((const int32_t *)codes.values)[i] : kNullRow;
}

static int env_int(const char *name, int lo, int hi, int dflt) {
    const char *e = std::getenv(name);
    if (!e || !*e) return dflt;
    const long v = std::strtol(e, nullptr, 10);
    return (int)std::min<long>(hi, std::max<long>(lo, v));
}

static int ceil_log2(uint64_t x) {
    int b = 0;
    while (b < 63 && (1ull << b) < x) ++b;
    return b;
}

static qeh_column view_column(int dtype, void *values, int64_t n) {
    qeh_column c{};
    c.dtype = dtype;
    c.length = n;
    c.values = values;
    return c;
}

static int empty_dict(qeh_ctx *ctx, qeh_column *out) {
    std::memset(out, 0, sizeof(*out));
    out->dtype = QEH_DT_UTF8;
    out->owned = 1;
    void *o = nullptr, *d = nullptr;
    QEH_TRY(ctx->pool->alloc(8, &o));
    const int s = ctx->pool->alloc(8, &d);
    if (s != QEH_OK) {
        ctx->pool->free(o);
        return s;
    }
    out->offsets = (int32_t *)o;
    out->values = d;
    QEH_HIP(hipMemsetAsync(o, 0, 8, ctx->stream));
    return QEH_OK;
}

// (c): the permutation of the d representatives that puts their strings in ascending order
static int order_representatives(qeh_ctx *ctx, const DictIn &in, const uint32_t *rep_row, int64_t d, uint32_t *ctl,
                                 qeh_column *out_perm) {
    DevBuf word, rem, seg, flags, excl;
    QEH_TRY(word.alloc(ctx, (size_t)d * 8));
    QEH_TRY(rem.alloc(ctx, (size_t)d * 4));
    QEH_TRY(seg.alloc(ctx, (size_t)d * 4));
    QEH_TRY(flags.alloc(ctx, (size_t)d * 4));
    QEH_TRY(excl.alloc(ctx, (size_t)d * 8));
    const int grid = grid_for(ctx, d, kBlock, 8);
    const int8_t asc[3] = {1, 1, 1};
    uint32_t maxlen = 0;
    for (int64_t r = 0;; ++r) {
        {
            KernelTimer kt(ctx, "utf8_dict_order");
            hipLaunchKernelGGL(k_dict_pack, dim3(grid), dim3(kBlock), 0, ctx->stream, in, rep_row, d, (int32_t)(8 * r),
                               word.as<int64_t>(), rem.as<int32_t>(), r == 0 ? ctl : (uint32_t *)nullptr);
        }
        QEH_HIP(hipGetLastError());
        qeh_column keys[3] = {view_column(QEH_DT_INT32, seg.p, d), view_column(QEH_DT_INT64, word.p, d),
                              view_column(QEH_DT_INT32, rem.p, d)};
        // round 0: every representative is in segment 0
        QEH_TRY(r == 0 ? qeh_sort_indices(ctx, keys + 1, 2, asc, out_perm) : qeh_sort_indices(ctx, keys, 3, asc, out_perm));
        const uint32_t *perm = (const uint32_t *)out_perm->values;
        uint64_t segments = 0;
        {
            KernelTimer kt(ctx, "utf8_dict_order");
            hipLaunchKernelGGL(k_dict_flags, dim3(grid), dim3(kBlock), 0, ctx->stream, perm,
                               r == 0 ? (const int32_t *)nullptr : seg.as<int32_t>(), word.as<int64_t>(), rem.as<int32_t>(), d,
                               flags.as<uint32_t>());
        }
        int s = exclusive_scan_u32(ctx, flags.as<uint32_t>(), excl.as<uint64_t>(), d, &segments);
        if (s == QEH_OK && r == 0) s = read_small(ctx, &maxlen, ctl + DC_MAXLEN, 4);
        if (s != QEH_OK) {
            qeh_column_release(ctx, out_perm);
            return s;
        }
        // distinct strings differ within the longest length, so the second test only bounds the loop
        if ((int64_t)segments == d || 8 * (r + 1) >= (int64_t)maxlen) return QEH_OK;
        {
            KernelTimer kt(ctx, "utf8_dict_order");
            hipLaunchKernelGGL(k_dict_segments, dim3(grid), dim3(kBlock), 0, ctx->stream, perm, flags.as<uint32_t>(),
                               excl.as<uint64_t>(), d, seg.as<int32_t>());
        }
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
            qeh_column_release(ctx, out_perm);
            return fail(QEH_E_HIP, "utf8 dictionary: segment launch failed");
        }
        qeh_column_release(ctx, out_perm);
    }
}

static int dict_input(const qeh_column &col, const char *who, DictIn *in) {
    QEH_TRY(check_column(col, "utf8 dictionary"));
    if (col.dtype != QEH_DT_UTF8) return fail(QEH_E_INVALID, std::string(who) + ": the column is not Utf8");
    // representative rows are stored as 32-bit row + 1, slots and ranks as 32-bit words
    if (col.length >= (int64_t)0xFFFFFFFFll)
        return fail(QEH_E_UNSUPPORTED, "utf8 dictionary: more than 2^32-2 rows per column");
    if (col.length > 0 && !col.offsets) return fail(QEH_E_INVALID, std::string(who) + ": Utf8 column without offsets");
    in->valid = make_colref(col);
    in->offs = col.offsets + col.offset;
    in->data = (const uint8_t *)col.values;
    return QEH_OK;
}

// The test knobs, read once per call: every kernel of the call then masks its hashes alike.
struct DictKnobs {
    int cap_log2;  // first table size
    uint64_t hash_mask;
};
static DictKnobs dict_knobs() {
    const int hash_bits = env_int("QEH_UTF8_DICT_HASH_BITS", 1, 64, 64);
    return {env_int("QEH_UTF8_DICT_CAP_LOG2", 4, kDictMaxCapLog2, kDictDefaultCapLog2),
            hash_bits >= 64 ? ~0ull : (1ull << hash_bits) - 1ull};
}

// (a) and the scan of (b): the finished table of a column's distinct strings, the slot of every row
// and the dense id of every occupied slot (`dense` is left empty when there is no string at all).
struct DictTable {
    DevBuf table, slot_of_row, ctl, dense;
    uint64_t cap = 0;
    int cap_log2 = 0;
    int64_t distinct = 0;
};

static int build_dict_table(qeh_ctx *ctx, const DictIn &in, int64_t n, const DictKnobs &knobs, DictTable *dt) {
    DevBuf &table = dt->table, &slot_of_row = dt->slot_of_row;
    QEH_TRY(dt->ctl.alloc(ctx, DC_WORDS * 4));
    uint32_t *ctl = dt->ctl.as<uint32_t>();
    QEH_TRY(slot_of_row.alloc(ctx, (size_t)std::max<int64_t>(n, 1) * 4));
    // a table of 2n slots is never more than half full; below it a half-full table grows
    const int full_log2 = std::min(kDictMaxCapLog2, std::max(4, ceil_log2((uint64_t)std::max<int64_t>(n, 1) * 2)));
    int cap_log2 = std::min(full_log2, knobs.cap_log2);
    const uint64_t hash_mask = knobs.hash_mask;
    uint64_t cap = 0;
    uint32_t distinct = 0;
    int grows = 0;
    for (;;) {
        cap = 1ull << cap_log2;
        QEH_TRY(table.alloc(ctx, (size_t)cap * 8));
        QEH_HIP(hipMemsetAsync(table.p, 0, (size_t)cap * 8, ctx->stream));
        QEH_HIP(hipMemsetAsync(ctl, 0, DC_WORDS * 4, ctx->stream));
        const uint32_t limit = cap_log2 >= full_log2 ? 0x7FFFFFFFu : (uint32_t)(cap / 2);
        if (n > 0) {
            KernelTimer kt(ctx, "utf8_dict_insert");
            hipLaunchKernelGGL(k_dict_insert, dim3(grid_for(ctx, n, kBlock * 4, 8)), dim3(kBlock), 0, ctx->stream, in, n,
                               table.as<uint64_t>(), cap_log2, hash_mask, limit, slot_of_row.as<uint32_t>(), ctl);
        }
        QEH_HIP(hipGetLastError());
        uint32_t st[2] = {0, 0};
        QEH_TRY(read_small(ctx, st, ctl, 8));
        distinct = st[DC_COUNT];
        if (!st[DC_OVERFLOW]) break;
        if (cap_log2 >= full_log2) {
            // never more than half full, so a probe ran out of its kDictMaxProbe steps (strings that
            // share their whole hash); a larger table spreads the runs, twice at the most
            if (distinct >= 0x7FFFFFFFu)
                return fail(QEH_E_UNSUPPORTED, "utf8 dictionary: more than INT32_MAX distinct strings");
            if (cap_log2 >= kDictMaxCapLog2 || cap_log2 >= full_log2 + 8)
                return fail(QEH_E_UNSUPPORTED, "utf8 dictionary: a probe sequence ran out of steps at " +
                                                   std::to_string(cap) + " slots (too many strings share one hash)");
            cap_log2 = std::min(kDictMaxCapLog2, cap_log2 + 4);
        } else {
            // half full: 16x once (few distinct strings stay in L2), then the full size at once --
            // every aborted pass re-reads rows, and the passes just below the full size read most
            grows += 1;
            cap_log2 = grows >= 2 ? full_log2 : std::min(full_log2, cap_log2 + 4);
        }
    }
    dt->cap = cap;
    dt->cap_log2 = cap_log2;
    dt->distinct = (int64_t)distinct;
    if (distinct == 0) return QEH_OK;  // n == 0 or all NULL
    DevBuf occ;
    QEH_TRY(occ.alloc(ctx, (size_t)cap * 4));
    QEH_TRY(dt->dense.alloc(ctx, (size_t)cap * 8));
    uint64_t occupied = 0;
    {
        KernelTimer kt(ctx, "utf8_dict_compact");
        hipLaunchKernelGGL(k_dict_occupied, dim3(grid_for(ctx, (int64_t)cap, kBlock * 4, 8)), dim3(kBlock), 0, ctx->stream,
                           table.as<uint64_t>(), cap, occ.as<uint32_t>());
    }
    QEH_TRY(exclusive_scan_u32(ctx, occ.as<uint32_t>(), dt->dense.as<uint64_t>(), (int64_t)cap, &occupied));
    if ((int64_t)occupied != dt->distinct) return fail(QEH_E_INTERNAL, "utf8 dictionary: slot count mismatch");
    return QEH_OK;
}

static int utf8_dict_encode(qeh_ctx *ctx, const qeh_column &col, qeh_column *out_codes, qeh_column *out_dict) {
    DictIn in{};
    QEH_TRY(dict_input(col, "qeh_utf8_dict_encode", &in));
    const int64_t n = col.length;
    const bool nullable = col.validity != nullptr;
    DictTable dt;
    QEH_TRY(build_dict_table(ctx, in, n, dict_knobs(), &dt));
    DevBuf &table = dt.table, &slot_of_row = dt.slot_of_row, &dense = dt.dense;
    uint32_t *ctl = dt.ctl.as<uint32_t>();
    const uint64_t cap = dt.cap;
    const int64_t d = dt.distinct;

    QEH_TRY(alloc_column(ctx, QEH_DT_INT32, n, nullable, out_codes));
    auto bail = [&](int s) {
        qeh_column_release(ctx, out_codes);
        return s;
    };
    if (d == 0) {  // n == 0 or all NULL
        if (n > 0) {
            if (hipMemsetAsync(out_codes->values, 0, (size_t)n * 4, ctx->stream) != hipSuccess ||
                hipMemsetAsync(out_codes->validity, 0, (size_t)((n + 63) / 64) * 8, ctx->stream) != hipSuccess)
                return bail(fail(QEH_E_HIP, "utf8 dictionary: memset failed"));
        }
        int s = empty_dict(ctx, out_dict);
        if (s == QEH_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) s = fail(QEH_E_HIP, "utf8 dictionary failed");
        return s == QEH_OK ? s : bail(s);
    }

    DevBuf rep_row, sorted_row, rank_of_rep, rank_of_slot;
    int s = rep_row.alloc(ctx, (size_t)d * 4);
    if (s == QEH_OK) s = sorted_row.alloc(ctx, (size_t)d * 4);
    if (s == QEH_OK) s = rank_of_rep.alloc(ctx, (size_t)d * 4);
    if (s == QEH_OK) s = rank_of_slot.alloc(ctx, (size_t)cap * 4);
    if (s != QEH_OK) return bail(s);
    const int gcap = grid_for(ctx, (int64_t)cap, kBlock * 4, 8);
    {
        KernelTimer kt(ctx, "utf8_dict_compact");
        hipLaunchKernelGGL(k_dict_reps, dim3(gcap), dim3(kBlock), 0, ctx->stream, table.as<uint64_t>(), cap, dense.as<uint64_t>(),
                           rep_row.as<uint32_t>());
    }
    qeh_column perm{};
    s = order_representatives(ctx, in, rep_row.as<uint32_t>(), d, ctl, &perm);
    if (s != QEH_OK) return bail(s);
    {
        KernelTimer kt(ctx, "utf8_dict_codes");
        hipLaunchKernelGGL(k_dict_ranks, dim3(grid_for(ctx, d, kBlock * 4, 8)), dim3(kBlock), 0, ctx->stream,
                           (const uint32_t *)perm.values, rep_row.as<uint32_t>(), d, sorted_row.as<uint32_t>(),
                           rank_of_rep.as<uint32_t>());
        hipLaunchKernelGGL(k_dict_slot_ranks, dim3(gcap), dim3(kBlock), 0, ctx->stream, table.as<uint64_t>(), cap,
                           dense.as<uint64_t>(), rank_of_rep.as<uint32_t>(), rank_of_slot.as<uint32_t>());
        hipLaunchKernelGGL(k_dict_codes<uint32_t>, dim3(grid_for(ctx, (n + 63) / 64, kBlock / 64, 8)), dim3(kBlock), 0, ctx->stream, in.valid,
                           slot_of_row.as<uint32_t>(), rank_of_slot.as<uint32_t>(), n, (int32_t *)out_codes->values,
                           (uint64_t *)out_codes->validity);
    }
    if (hipGetLastError() != hipSuccess) s = fail(QEH_E_HIP, "utf8 dictionary: launch failed");
    if (s == QEH_OK) {
        qeh_column src = col;  // the representatives are valid rows: the dictionary carries no bitmap
        src.validity = nullptr;
        src.null_count = 0;
        s = gather_column(ctx, src, sorted_row.as<uint32_t>(), d, out_dict);
    }
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && s == QEH_OK) {
        qeh_column_release(ctx, out_dict);
        s = fail(QEH_E_HIP, "utf8 dictionary failed");
    }
    qeh_column_release(ctx, &perm);
    if (s != QEH_OK) return bail(s);
    out_codes->null_count = nullable ? col.null_count : 0;
    return QEH_OK;
}

int utf8_join_encode(qeh_ctx *ctx, const qeh_column &build, const qeh_column &probe, qeh_column *out_build_codes,
                     qeh_column *out_probe_codes, int64_t *out_distinct) {
    DictIn bin{}, pin{};
    QEH_TRY(dict_input(build, "qeh_utf8_join_encode", &bin));
    QEH_TRY(dict_input(probe, "qeh_utf8_join_encode", &pin));
    const int64_t nb = build.length, np = probe.length;
    const DictKnobs knobs = dict_knobs();
    DictTable dt;
    QEH_TRY(build_dict_table(ctx, bin, nb, knobs, &dt));
    const int64_t d = dt.distinct;

    QEH_TRY(alloc_column(ctx, QEH_DT_INT32, nb, build.validity != nullptr, out_build_codes));
    int s = alloc_column(ctx, QEH_DT_INT32, np, true, out_probe_codes);
    if (s != QEH_OK) {
        qeh_column_release(ctx, out_build_codes);
        return s;
    }
    if (d == 0) {  // no build string: nothing matches
        bool ok = hipMemsetAsync(out_probe_codes->values, 0, (size_t)std::max<int64_t>(np, 1) * 4, ctx->stream) == hipSuccess &&
                  hipMemsetAsync(out_probe_codes->validity, 0, (size_t)std::max<int64_t>((np + 63) / 64, 1) * 8, ctx->stream) ==
                      hipSuccess;
        if (ok && nb > 0)  // all NULL, so the column has a bitmap
            ok = hipMemsetAsync(out_build_codes->values, 0, (size_t)nb * 4, ctx->stream) == hipSuccess &&
                 hipMemsetAsync(out_build_codes->validity, 0, (size_t)((nb + 63) / 64) * 8, ctx->stream) == hipSuccess;
        if (!ok) s = fail(QEH_E_HIP, "utf8 join dictionary: memset failed");
    } else {
        {
            KernelTimer kt(ctx, "utf8_dict_codes");
            hipLaunchKernelGGL(k_dict_codes<uint64_t>, dim3(grid_for(ctx, (nb + 63) / 64, kBlock / 64, 8)), dim3(kBlock), 0,
                               ctx->stream, bin.valid, dt.slot_of_row.as<uint32_t>(), dt.dense.as<uint64_t>(), nb,
                               (int32_t *)out_build_codes->values, (uint64_t *)out_build_codes->validity);
        }
        if (np > 0) {
            KernelTimer kt(ctx, "utf8_dict_lookup");
            hipLaunchKernelGGL(k_dict_lookup, dim3(grid_for(ctx, (np + 63) / 64, kBlock / 64, 8)), dim3(kBlock), 0, ctx->stream,
                               pin, np, bin, dt.table.as<uint64_t>(), dt.cap_log2, knobs.hash_mask, dt.dense.as<uint64_t>(),
                               (int32_t *)out_probe_codes->values, (uint64_t *)out_probe_codes->validity);
        }
        if (hipGetLastError() != hipSuccess) s = fail(QEH_E_HIP, "utf8 join dictionary: launch failed");
    }
    // the table and the dense ids are freed on return
    if (hipStreamSynchronize(ctx->stream) != hipSuccess && s == QEH_OK) s = fail(QEH_E_HIP, "utf8 join dictionary failed");
    if (s != QEH_OK) {
        qeh_column_release(ctx, out_build_codes);
        qeh_column_release(ctx, out_probe_codes);
        return s;
    }
    out_build_codes->null_count = build.validity ? build.null_count : 0;
    if (out_distinct) *out_distinct = d;
    return QEH_OK;
}

Utf8Keys::~Utf8Keys() {
    if (!ctx) return;
    for (auto &c : codes) qeh_column_release(ctx, &c);
    for (auto &c : dicts) qeh_column_release(ctx, &c);
}

int encode_utf8_keys(qeh_ctx *ctx, const qeh_column *keys, int n_keys, Utf8Keys *out) {
    out->ctx = ctx;
    out->keys.assign(keys, keys + std::max(n_keys, 0));
    out->dict_of_key.assign((size_t)std::max(n_keys, 0), -1);
    out->logical.assign((size_t)std::max(n_keys, 0), 0);
    for (int i = 0; i < n_keys; ++i) {
        out->logical[i] = keys[i].dtype;
        if (is_temporal(keys[i].dtype)) out->keys[i] = physical_view(keys[i]);
        if (keys[i].dtype != QEH_DT_UTF8) continue;
        qeh_column codes{}, dict{};
        QEH_TRY(utf8_dict_encode(ctx, keys[i], &codes, &dict));
        out->dict_of_key[i] = (int)out->dicts.size();
        out->codes.push_back(codes);
        out->dicts.push_back(dict);
        out->keys[i] = codes;
        out->keys[i].owned = 0;
    }
    return QEH_OK;
}

int Utf8Keys::decode(int key, qeh_column *col) const {
    if (key < 0 || key >= (int)dict_of_key.size()) return QEH_OK;
    if (is_temporal(logical[key]) && col->dtype == physical_dtype(logical[key])) col->dtype = logical[key];
    if (dict_of_key[key] < 0) return QEH_OK;
    const qeh_column &dict = dicts[dict_of_key[key]];
    const int64_t g = col->length;
    DevBuf idx;
    QEH_TRY(idx.alloc(ctx, (size_t)std::max<int64_t>(g, 1) * 4));
    if (g > 0)
        hipLaunchKernelGGL(k_dict_code_idx, dim3(grid_for(ctx, g, kBlock * 4, 8)), dim3(kBlock), 0, ctx->stream, make_colref(*col), g,
                           idx.as<uint32_t>());
    QEH_HIP(hipGetLastError());
    qeh_column strs{};
    QEH_TRY(gather_column(ctx, dict, idx.as<uint32_t>(), g, &strs, col->validity != nullptr));
    QEH_HIP(hipStreamSynchronize(ctx->stream));
    qeh_column_release(ctx, col);
    *col = strs;
    return QEH_OK;
}

}  // namespace qeh

using namespace qeh;

extern "C" int qeh_utf8_dict_encode(qeh_ctx *ctx, const qeh_column *col, qeh_column *out_codes, qeh_column *out_dict) {
    if (!ctx || !col || !out_codes || !out_dict) return fail(QEH_E_INVALID, "qeh_utf8_dict_encode: bad argument");
    DeviceGuard dg(ctx->device);
    return utf8_dict_encode(ctx, *col, out_codes, out_dict);
}

extern "C" int qeh_utf8_join_encode(qeh_ctx *ctx, const qeh_column *build, const qeh_column *probe,
                                    qeh_column *out_build_codes, qeh_column *out_probe_codes, int64_t *out_distinct) {
    if (!ctx || !build || !probe || !out_build_codes || !out_probe_codes)
        return fail(QEH_E_INVALID, "qeh_utf8_join_encode: bad argument");
    DeviceGuard dg(ctx->device);
    return utf8_join_encode(ctx, *build, *probe, out_build_codes, out_probe_codes, out_distinct);
}
