// Semi / anti join as an expression: `x [NOT] IN (set)` -> one bit per probe row.
//
// Reference: PhysicalExpr::InSubquery { expr, plan, negated } (crates/query-executor/src/
// physical_plan.rs:95-99) is produced by the planner and answered by the executor with "not yet
// implemented in synchronous context" (operators.rs:34-52); this is its intended semantics, SQL
// three-valued logic:
//   set has no rows at all                    -> negated ? TRUE : FALSE, valid, also for NULL probes
//   NULL probe (non-empty set)                -> NULL
//   found (probe valid)                       -> !negated
//   not found (probe valid), set has a NULL   -> NULL
//   not found (probe valid), set has no NULL  -> negated
// Keys compare by value bits (the project's `=` on keys): Int32 / Int64 widened to
// 64 bits, Float32 / Float64 by their bit patterns (same-bits NaN matches, 0.0 and -0.0 differ),
// Utf8 through the codes of one dictionary built over the set (utf8_join_encode).
//
// None of the join kernels fits: they materialise pairs or aggregate.  Here the set becomes either
//   a BITMAP, one bit per key offset k - min over the valid set keys' [min, max]: set by
//     non-returning atomicOr on 32-bit words (many keys share a word, plain stores would lose bits), or
//   a key-only HASH SET: 8-B slots, power-of-two capacity >= 2 * set rows (load <= 0.5), linear
//     probing, atomicCAS insert; the empty slot is a reserved value and the one key equal to it is a
//     side flag; duplicates collapse in the CAS.  No payload and no multi-match probing (which is
//     what build_join_table would switch on for a set with duplicates),
// and one streaming probe kernel writes the bit-packed BOOL column and its validity bitmap, one
// ballot word per 64 rows -- the layout k_utf8_cmp writes.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>

#include "device_common.h"
#include "ops.h"

namespace qeh {

constexpr uint64_t kSemiEmpty = ~0ull;          // hash set: empty slot (the key with these bits: a side flag)
constexpr int kSemiKeys = 4;                    // keys per lane per step
constexpr int kSemiTile = kWave * kSemiKeys;    // rows per wave step = 4 whole output words
enum SemiForm : int { SEMI_BITMAP = 0, SEMI_HASH = 1 };

// Which form (decided on the host from the valid set keys' range and count).  Derivation, not a
// measurement -- no run has compared the two forms:
//   footprint: the bitmap takes range / 8 bytes, the hash set 16 B per key (8-B slots at load 0.5).
//   probe:     the bitmap is one 4-B read at a computed offset; the hash set hashes, reads >= 1 8-B
//              slot and may walk a chain.
//   So while the bitmap is no larger than the hash set (range / 8 <= 16 nv, i.e. range <= 128 nv) it
//   is ahead on every count.  A sparser range still takes the bitmap while it stays within one
//   XCD's 4 MiB L2 (2^25 bits): every probe is then a cache hit and the build's memset is noise.
//   Above both bounds the bitmap would spill a cache the hash set still fits, so the hash set it is.
//   The bitmap is capped at 2^31 bits (256 MiB) whatever the row count.
constexpr uint64_t kSemiBitmapMaxBits = 1ull << 31;
constexpr uint64_t kSemiBitmapL2Bits = 1ull << 25;
// range = max - min + 1 of the valid keys as uint64 (0: the range overflows 64 bits)
__host__ __device__ inline bool semi_bitmap_fits(uint64_t range) { return range != 0 && range <= kSemiBitmapMaxBits; }
__host__ __device__ inline bool semi_bitmap_ok(uint64_t range, uint64_t nv) {
    if (!semi_bitmap_fits(range)) return false;
    return range <= kSemiBitmapL2Bits || range / 128 <= nv;
}

struct SemiSet {
    const uint32_t *bits;   // BITMAP: bit (k - mn)
    const uint64_t *slots;  // HASH: keys, kSemiEmpty = empty
    uint64_t mask;          // HASH: capacity - 1
    uint64_t range;         // BITMAP: mx - mn + 1
    int64_t mn, mx;         // valid set keys' range: a probe key outside it is answered without a lookup
    int32_t has_empty_key;  // HASH: the key whose bits are kSemiEmpty is in the set
    int32_t has_null;       // the set holds a NULL
    int32_t negated;
    int32_t _pad;
};

// A key as 64 bits: 4-byte elements (Int32, Float32 bits, dictionary codes) sign-extended.
template <int W>
__device__ __forceinline__ int64_t semi_key(const void *v, int64_t row) {
    if (W == 4) return (int64_t)((const int32_t *)v)[row];
    return ((const int64_t *)v)[row];
}

template <int W>
__global__ void k_semi_build_bitmap(const void *__restrict__ vals, const uint8_t *__restrict__ valid, int64_t vbit0,
                                    int64_t n, int64_t mn, uint64_t range, uint32_t *__restrict__ bits) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (valid && !bit_at(valid, vbit0 + i)) continue;
        const uint64_t off = (uint64_t)semi_key<W>(vals, i) - (uint64_t)mn;
        if (off < range)  // always, by the min/max read; keeps a store inside the bitmap regardless
            (void)__hip_atomic_fetch_or(&bits[off >> 5], 1u << (off & 31), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// flags[0]: the key equal to kSemiEmpty occurs; flags[1]: an insert found no slot (cannot happen at
// load <= 0.5; reported as QEH_E_INTERNAL).  *nvalid += the non-NULL rows.
template <int W>
__global__ void k_semi_build_hash(const void *__restrict__ vals, const uint8_t *__restrict__ valid, int64_t vbit0,
                                  int64_t n, uint64_t *__restrict__ slots, uint64_t mask, uint32_t *__restrict__ flags,
                                  unsigned long long *__restrict__ nvalid) {
    uint64_t cnt = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        if (valid && !bit_at(valid, vbit0 + i)) continue;
        ++cnt;
        const uint64_t key = (uint64_t)semi_key<W>(vals, i);
        if (key == kSemiEmpty) {
            atomicOr(&flags[0], 1u);
            continue;
        }
        uint64_t h = hash64(key) & mask;
        bool placed = false;
        for (uint64_t step = 0; step <= mask; ++step) {
            const uint64_t prev = atomicCAS((unsigned long long *)&slots[h], (unsigned long long)kSemiEmpty,
                                            (unsigned long long)key);
            if (prev == kSemiEmpty || prev == key) {  // inserted, or a duplicate: already there
                placed = true;
                break;
            }
            h = (h + 1) & mask;
        }
        if (!placed) atomicOr(&flags[1], 1u);
    }
    cnt = wave_sum_u64(cnt);
    if (lane_id() == 0 && cnt) atomicAdd(nvalid, (unsigned long long)cnt);
}

template <int FORM>
__device__ __forceinline__ bool semi_lookup(const SemiSet &s, int64_t key) {
    if (FORM == SEMI_BITMAP) {
        const uint64_t off = (uint64_t)key - (uint64_t)s.mn;  // a key below mn wraps past range
        if (off >= s.range) return false;
        return (s.bits[off >> 5] >> (off & 31)) & 1u;
    }
    if (key < s.mn || key > s.mx) return false;
    if ((uint64_t)key == kSemiEmpty) return s.has_empty_key != 0;
    uint64_t h = hash64((uint64_t)key) & s.mask;
    for (uint64_t i = 0; i <= s.mask; ++i) {
        const uint64_t e = s.slots[h];
        if (e == (uint64_t)key) return true;
        if (e == kSemiEmpty) return false;
        h = (h + 1) & s.mask;
    }
    return false;
}

// Bit i of x (i < 64 / E) to bit E * i: a lane holds E consecutive rows, so the ballot of its e-th
// row carries every E-th bit of an output word.
template <int E>
__host__ __device__ __forceinline__ uint64_t semi_spread(uint64_t x) {
    if (E == 2) {
        x &= 0xFFFFFFFFull;
        x = (x | (x << 16)) & 0x0000FFFF0000FFFFull;
        x = (x | (x << 8)) & 0x00FF00FF00FF00FFull;
        x = (x | (x << 4)) & 0x0F0F0F0F0F0F0F0Full;
        x = (x | (x << 2)) & 0x3333333333333333ull;
        x = (x | (x << 1)) & 0x5555555555555555ull;
        return x;
    }
    x &= 0xFFFFull;
    x = (x | (x << 24)) & 0x000000FF000000FFull;
    x = (x | (x << 12)) & 0x000F000F000F000Full;
    x = (x | (x << 6)) & 0x0303030303030303ull;
    x = (x | (x << 3)) & 0x1111111111111111ull;
    return x;
}

typedef long long semi_v2i64 __attribute__((ext_vector_type(2)));
typedef int semi_v4i32 __attribute__((ext_vector_type(4)));

// One wave step = kSemiTile rows = 4 whole output words, so no two waves write one word.  A lane
// holds kSemiKeys keys from 16-B loads (E = 16 / W keys each): row = base + u * 64 E + E * lane + e.
// `vec` (host-checked: the first value 16-B aligned) lets full tiles take the 16-B loads; a partial
// last tile, or an unaligned column, reads its rows one by one in the same lane layout, rows >= n
// not at all (they contribute 0 bits).  `present` (Utf8: the validity of the probe's dictionary
// codes): a valid probe row with its bit cleared is absent from the set without a lookup.
template <int FORM, int W>
__global__ void __launch_bounds__(kBlock)
k_semi_probe(const void *__restrict__ vals, const uint8_t *__restrict__ valid, int64_t vbit0,
             const uint8_t *__restrict__ present, int64_t pbit0, int64_t n, int vec, SemiSet s,
             uint64_t *__restrict__ out_bits, uint64_t *__restrict__ out_valid) {
    constexpr int E = 16 / W;
    constexpr int U = kSemiKeys / E;
    constexpr int LW = 64 / E;  // lanes per output word
    const int lane = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * (kBlock / 64);
    const int64_t ntiles = (n + kSemiTile - 1) / kSemiTile, nwords = (n + 63) / 64;
    for (int64_t t = (int64_t)blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6); t < ntiles; t += nwaves) {
        const int64_t base = t * kSemiTile;
        int64_t key[U][E];
        if (vec && base + kSemiTile <= n) {  // wave-uniform
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int64_t r = base + (int64_t)u * 64 * E + E * lane;
                if (W == 8) {
                    const semi_v2i64 x = __builtin_nontemporal_load((const semi_v2i64 *)((const int64_t *)vals + r));
                    key[u][0] = x[0], key[u][E - 1] = x[1];
                } else {
                    const semi_v4i32 x = __builtin_nontemporal_load((const semi_v4i32 *)((const int32_t *)vals + r));
#pragma unroll
                    for (int e = 0; e < E; ++e) key[u][e] = (int64_t)x[e];
                }
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int e = 0; e < E; ++e) {
                    const int64_t r = base + (int64_t)u * 64 * E + E * lane + e;
                    key[u][e] = r < n ? semi_key<W>(vals, r) : 0;
                }
        }
        uint64_t rb[U][E], vb[U][E];
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int e = 0; e < E; ++e) {
                const int64_t r = base + (int64_t)u * 64 * E + E * lane + e;
                const bool pv = r < n && (!valid || bit_at(valid, vbit0 + r));
                const bool cand = pv && (!present || bit_at(present, pbit0 + r));
                const bool found = cand && semi_lookup<FORM>(s, key[u][e]);
                const bool ov = pv && (found || !s.has_null);
                rb[u][e] = __ballot(ov && (found != (s.negated != 0)));
                vb[u][e] = __ballot(ov);
            }
        // word w of the tile = load w / E, lanes [(w % E) LW, (w % E + 1) LW)
        uint64_t mine_r = 0, mine_v = 0;
#pragma unroll
        for (int w = 0; w < kSemiKeys; ++w) {
            const int u = w / E, q = w % E;
            uint64_t wr = 0, wv = 0;
#pragma unroll
            for (int e = 0; e < E; ++e) {
                wr |= semi_spread<E>(rb[u][e] >> (q * LW)) << e;
                wv |= semi_spread<E>(vb[u][e] >> (q * LW)) << e;
            }
            if (lane == w) mine_r = wr, mine_v = wv;
        }
        const int64_t w0 = t * kSemiKeys;
        if (lane < kSemiKeys && w0 + lane < nwords) {
            out_bits[w0 + lane] = mine_r;
            if (out_valid) out_valid[w0 + lane] = mine_v;
        }
    }
}

static int forced_in_set_form() {  // read per call: tests switch it between calls
    const char *e = std::getenv("QEH_IN_SET");
    if (!e) return -1;
    if (!std::strcmp(e, "bitmap")) return SEMI_BITMAP;
    if (!std::strcmp(e, "hash")) return SEMI_HASH;
    return -1;
}

static bool semi_int(int dt) { return dt == QEH_DT_INT32 || dt == QEH_DT_INT64; }

// every row the same valid value (`value`), or every row NULL (`null`)
static int semi_constant(qeh_ctx *ctx, int64_t n, bool value, bool null, qeh_column *out) {
    QEH_TRY(alloc_column(ctx, QEH_DT_BOOL, n, null, out));
    const size_t bytes = (size_t)((n + 63) / 64) * 8;
    if (bytes) QEH_HIP(hipMemsetAsync(out->values, 0, bytes, ctx->stream));
    if (null && bytes) QEH_HIP(hipMemsetAsync(out->validity, 0, bytes, ctx->stream));
    if (value && !null && n > 0) {  // whole bytes, then the low bits of a last partial one
        if (n / 8) QEH_HIP(hipMemsetAsync(out->values, 0xFF, (size_t)(n / 8), ctx->stream));
        if (n % 8) QEH_HIP(hipMemsetAsync((uint8_t *)out->values + n / 8, (1 << (n % 8)) - 1, 1, ctx->stream));
    }
    out->null_count = null ? n : 0;
    return QEH_OK;
}

// The integer path: n probe values `pc` of width pw = 4 / 8 against the set column of width 4 / 8.
// `is_int`: the keys are integers (a min/max range exists, so the bitmap is eligible).
static int semi_run(qeh_ctx *ctx, const ColRef &pc, int pw, int64_t n, const uint8_t *present, int64_t pbit0,
                    const qeh_column &set, bool is_int, int negated, qeh_column *out) {
    const int64_t m = set.length;
    const int sw = (int)dtype_size(set.dtype);
    const ColRef sc = make_colref(set);
    SemiSet s{};
    s.negated = negated ? 1 : 0;
    s.mn = INT64_MIN, s.mx = INT64_MAX;
    int64_t nv = -1;
    int form = SEMI_HASH;
    const int forced = forced_in_set_form();
    if (is_int) {
        QEH_TRY(column_minmax(ctx, set, &s.mn, &s.mx, &nv));
        if (nv == 0) return semi_constant(ctx, n, false, true, out);  // only NULLs in the set: nothing is found
        const uint64_t range = (uint64_t)s.mx - (uint64_t)s.mn + 1ull;
        if (forced == SEMI_BITMAP && !semi_bitmap_fits(range))
            return fail(QEH_E_INVALID, "QEH_IN_SET=bitmap: the set's key range does not fit a bitmap");
        form = forced >= 0 ? forced : (semi_bitmap_ok(range, (uint64_t)nv) ? SEMI_BITMAP : SEMI_HASH);
        s.range = range;
    }
    DevBuf table, flags;
    const int bgrid = grid_for(ctx, m, kBlock * 4, 8);
    if (form == SEMI_BITMAP) {
        const size_t words = (size_t)((s.range + 31) / 32);
        QEH_TRY(table.alloc(ctx, words * 4));
        QEH_HIP(hipMemsetAsync(table.p, 0, words * 4, ctx->stream));
        {
            KernelTimer kt(ctx, "semi_build_bitmap");
            if (sw == 4)
                hipLaunchKernelGGL(k_semi_build_bitmap<4>, dim3(bgrid), dim3(kBlock), 0, ctx->stream, sc.values, sc.validity,
                                   sc.vbit0, m, s.mn, s.range, table.as<uint32_t>());
            else
                hipLaunchKernelGGL(k_semi_build_bitmap<8>, dim3(bgrid), dim3(kBlock), 0, ctx->stream, sc.values, sc.validity,
                                   sc.vbit0, m, s.mn, s.range, table.as<uint32_t>());
        }
        QEH_HIP(hipGetLastError());
        s.bits = table.as<uint32_t>();
    } else {
        uint64_t cap = 64;
        while (cap < 2 * (uint64_t)m) cap <<= 1;
        QEH_TRY(table.alloc(ctx, (size_t)cap * 8));
        QEH_HIP(hipMemsetAsync(table.p, 0xFF, (size_t)cap * 8, ctx->stream));
        QEH_TRY(flags.alloc(ctx, 16));
        QEH_HIP(hipMemsetAsync(flags.p, 0, 16, ctx->stream));
        {
            KernelTimer kt(ctx, "semi_build_hash");
            if (sw == 4)
                hipLaunchKernelGGL(k_semi_build_hash<4>, dim3(bgrid), dim3(kBlock), 0, ctx->stream, sc.values, sc.validity,
                                   sc.vbit0, m, table.as<uint64_t>(), cap - 1, flags.as<uint32_t>(),
                                   (unsigned long long *)(flags.as<uint64_t>() + 1));
            else
                hipLaunchKernelGGL(k_semi_build_hash<8>, dim3(bgrid), dim3(kBlock), 0, ctx->stream, sc.values, sc.validity,
                                   sc.vbit0, m, table.as<uint64_t>(), cap - 1, flags.as<uint32_t>(),
                                   (unsigned long long *)(flags.as<uint64_t>() + 1));
        }
        QEH_HIP(hipGetLastError());
        uint64_t fl[2];
        QEH_TRY(read_small(ctx, fl, flags.p, 16));
        if ((fl[0] >> 32) & 1u) return fail(QEH_E_INTERNAL, "in_set: hash set insert found no slot");
        s.has_empty_key = (int32_t)(fl[0] & 1u);
        if (nv < 0) nv = (int64_t)fl[1];
        if (nv == 0) return semi_constant(ctx, n, false, true, out);
        s.slots = table.as<uint64_t>();
        s.mask = cap - 1;
    }
    s.has_null = nv < m ? 1 : 0;
    QEH_TRY(alloc_column(ctx, QEH_DT_BOOL, n, pc.validity != nullptr || s.has_null, out));
    const int vec = ((uintptr_t)pc.values & 15) == 0 ? 1 : 0;
    const int grid = grid_for(ctx, n, kSemiTile * (kBlock / 64), 8);
    {
        KernelTimer kt(ctx, form == SEMI_BITMAP ? "semi_probe_bitmap" : "semi_probe_hash");
#define QEH_SEMI_PROBE(F, W)                                                                                          \
    hipLaunchKernelGGL((k_semi_probe<F, W>), dim3(grid), dim3(kBlock), 0, ctx->stream, pc.values, pc.validity, pc.vbit0, \
                       present, pbit0, n, vec, s, (uint64_t *)out->values, (uint64_t *)out->validity)
        if (form == SEMI_BITMAP) {
            if (pw == 4) QEH_SEMI_PROBE(SEMI_BITMAP, 4);
            else QEH_SEMI_PROBE(SEMI_BITMAP, 8);
        } else {
            if (pw == 4) QEH_SEMI_PROBE(SEMI_HASH, 4);
            else QEH_SEMI_PROBE(SEMI_HASH, 8);
        }
#undef QEH_SEMI_PROBE
    }
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the set's buffers return to the pool with this frame
    if (e != hipSuccess) {
        qeh_column_release(ctx, out);
        return fail(QEH_E_HIP, std::string("in_set: probe: ") + hipGetErrorString(e));
    }
    out->null_count = out->validity ? -1 : 0;
    return QEH_OK;
}

int in_set(qeh_ctx *ctx, const qeh_column &probe, const qeh_column &set, int negated, qeh_column *out) {
    std::memset(out, 0, sizeof(*out));
    QEH_TRY(check_column(probe, "in_set probe"));
    QEH_TRY(check_column(set, "in_set set"));
    if (probe.dtype == set.dtype && is_temporal(probe.dtype))  // the same temporal type: its physical integers
        return in_set(ctx, physical_view(probe), physical_view(set), negated, out);
    const int pt = probe.dtype, st = set.dtype;
    const bool ints = semi_int(pt) && semi_int(st);
    const bool floats = pt == st && (pt == QEH_DT_FLOAT32 || pt == QEH_DT_FLOAT64);
    const bool strs = pt == QEH_DT_UTF8 && st == QEH_DT_UTF8;
    if (!ints && !floats && !strs)  // what arrow's eq kernel says of the pair
        return fail(QEH_E_TYPE, std::string("Invalid argument error: Invalid comparison operation: ") +
                                    arrow_type_name(pt) + " == " + arrow_type_name(st));
    const int64_t n = probe.length;
    if (n == 0) return semi_constant(ctx, 0, false, false, out);
    if (set.length == 0) return semi_constant(ctx, n, negated != 0, false, out);  // even for NULL probes
    if (!strs) return semi_run(ctx, make_colref(probe), (int)dtype_size(pt), n, nullptr, 0, set, ints, negated, out);
    // Utf8: the unordered codes of one dictionary built over the set, then the integer path.  A
    // probe string the set lacks has no code (its code row is NULL): `present` tells it from a
    // NULL probe, whose answer is NULL.
    qeh_column bc{}, pcodes{};
    QEH_TRY(utf8_join_encode(ctx, set, probe, &bc, &pcodes, nullptr));
    ColRef pc = make_colref(pcodes);  // the codes' values under the probe column's own validity
    pc.validity = probe.validity;
    pc.vbit0 = probe.offset;
    const int s = semi_run(ctx, pc, 4, n, pcodes.validity, pcodes.offset, bc, true, negated, out);
    qeh_column_release(ctx, &bc);
    qeh_column_release(ctx, &pcodes);
    return s;
}

}  // namespace qeh

extern "C" int qeh_in_set(qeh_ctx *ctx, const qeh_column *probe, const qeh_column *set, int negated, qeh_column *out) {
    if (!ctx || !probe || !set || !out) return qeh::fail(QEH_E_INVALID, "qeh_in_set: bad argument");
    qeh::DeviceGuard dg(ctx->device);
    return qeh::in_set(ctx, *probe, *set, negated, out);
}
