// Device-side definitions the aggregate units share (k_aggregate.hip, k_agg_probe.hip, k_slice_join.hip,
// k_agg_fused.hip): tile constants, the group-id source, the unique
// table probe, the LDS-slice pipeline's shapes and plans, the finalize kernels' output columns.
#pragma once
#include "agg.h"
#include "expr_device.h"
#include "fast_tile.h"
#include "ops.h"

namespace qeh {

constexpr int kAggR = 4;                           // rows per lane
constexpr int kAggTile = kBlock * kAggR;           // rows per workgroup iteration
constexpr size_t kLdsStateBudget = 48 * 1024;      // bytes of LDS state per workgroup
constexpr int kFastTile = kBlock * kFastR;         // 2048 rows per fast-path workgroup iteration

enum GidMode { GM_ZERO = 0, GM_JOIN = 1, GM_GROUP = 2, GM_LDSHASH = 3 };
enum PredMode { PM_NONE = 0, PM_TERMS = 1, PM_PROG = 2 };

constexpr int64_t kEmptyKey = INT64_MIN;
struct GTable {                  // GM_LDSHASH: HBM table of group keys (EMPTY = INT64_MIN)
    int64_t *keys;
    uint64_t mask;               // capacity - 1; states index gcap = NULL group, gcap+1 = key INT64_MIN
    uint32_t *overflow;
};

struct GidSource {
    HashTable jt;            // GM_JOIN
    int32_t key_col;         // GM_JOIN: probe key column in the ColSet
    int32_t _pad;
    KeyCols gk;              // GM_GROUP: key columns (absolute ColRefs)
    const uint32_t *gslots;  // GM_GROUP
    uint64_t gmask;
    const uint64_t *gdense;
    GTable gt;               // GM_LDSHASH
    int32_t lcap;            // GM_LDSHASH: LDS slots per workgroup
    int32_t _pad2;
};

// Global states are kept in specs.shards copies ([shard][slot][G]); workgroup b
// merges into copy b % shards, so thousands of workgroups do not all hit the
// same few KB with atomics.  k_states_reduce folds the copies into copy 0.
__device__ __forceinline__ uint64_t *shard_states(uint64_t *all, const AggSpecs &specs, int64_t G) {
    return all + (uint64_t)(blockIdx.x % (unsigned)specs.shards) * (uint64_t)specs.n_slots * (uint64_t)G;
}

// ---- the fast kernels' shared pieces: the unique-table probe and the LDS state update ----
// One key looked up in a unique join table of any layout: true with its payload (the group id) in gid.
__device__ __forceinline__ bool probe_unique(const HashTable &t, int64_t key, uint32_t &gid) {
    if (key < t.kmin || key > t.kmax) return false;
    if (t.kind == TK_DIRECT) {
        const uint64_t i = (uint64_t)key - (uint64_t)t.kmin;
        uint32_t e = t.payload16 ? (uint32_t)t.payload16[i] : t.payload[i];
        gid = e - 1u;
        return e != 0;
    }
    if (t.kind == TK_BUCKET) {
        const int S = bucket_slots(t.pbits);
        uint64_t b = bucket_home(t, (uint64_t)key);
        for (uint64_t step = 0; step < t.nbkt; ++step) {
            uint64_t w[8];
            bucket_load(t, b, w);
            const uint32_t cnt = (uint32_t)(w[7] >> 32);
            // every slot compared with constant register indices (a runtime slot index into w
            // costs a chain of selects per access), the payload picked the same way
            uint32_t hit = 0;
#pragma unroll
            for (int s = 0; s < 6; ++s) hit |= (s < S && s < (int)cnt && (int64_t)w[s] == key) ? 1u << s : 0u;
            if (hit) {
                const int s0 = __builtin_ctz(hit);
                uint32_t pl = 0;
#pragma unroll
                for (int s = 0; s < 6; ++s)
                    if (s == s0) pl = bucket_payload(w, s, t.pbits);
                gid = pl - 1u;
                return true;
            }
            if (cnt <= (uint32_t)S) return false;
            b = b + 1 == t.nbkt ? 0 : b + 1;
        }
        return false;
    }
    uint64_t h = hash64((uint64_t)key) & t.mask;
    if (t.kind == TK_WIDE) {
        for (uint64_t i = 0; i <= t.mask; ++i) {
            const v2u64 e = wide_slot(t, h);
            if (e[1] == 0) return false;
            if ((int64_t)e[0] == key) {
                gid = (uint32_t)(e[1] - 1ull);
                return true;
            }
            h = (h + 1) & t.mask;
        }
        return false;
    }
    const uint64_t want = (uint64_t)key - (uint64_t)t.kmin + 1ull;
    for (uint64_t i = 0; i <= t.mask; ++i) {
        uint64_t e = t.slots[h];
        if (e == 0) return false;
        if ((e >> t.pbits) == want) {
            gid = (uint32_t)(e & ((1ull << t.pbits) - 1ull));
            return true;
        }
        h = (h + 1) & t.mask;
    }
    return false;
}

// Apply one tile's rows (mask m, LDS state slot per row) to LDS states laid
// out [value slot][stride] with row counts in slot 0.  Aggregate kinds are
// uniform, so the switch sits outside the row loop and each aggregate's LDS
// atomics for the tile's rows issue back to back.
template <int NTERMS, int NACOL, bool NT>
__device__ __forceinline__ void lds_apply_rows(uint64_t *lds, int64_t stride, const AggSpecs &specs, const FastIn &in,
                                               const FastTile<NTERMS, NACOL, NT> &ft, uint32_t m, const int *slot) {
#pragma unroll
    for (int r = 0; r < kFastR; ++r)
        if ((m >> r) & 1) atomicAdd((unsigned long long *)&lds[slot[r]], 1ull);
    for (int a = 0; a < specs.n; ++a) {
        const AggSpec sp = specs.a[a];
        uint64_t *st = lds + (int64_t)sp.val_slot * stride;
        const int cs = in.agg_colslot[a];
        switch (sp.kind) {
            case AK_SUM_F:
#pragma unroll
                for (int r = 0; r < kFastR; ++r)
                    if ((m >> r) & 1) atomicAdd((double *)&st[slot[r]], as_f64(ft.a(cs, r)));
                break;
            case AK_SUM_I:
#pragma unroll
                for (int r = 0; r < kFastR; ++r)
                    if ((m >> r) & 1) atomicAdd((unsigned long long *)&st[slot[r]], (unsigned long long)ft.a(cs, r));
                break;
            case AK_MIN:
            case AK_MAX:
#pragma unroll
                for (int r = 0; r < kFastR; ++r)
                    if ((m >> r) & 1) agg_apply<true>(sp.kind, &st[slot[r]], agg_input(sp.kind, sp.in_type, ft.a(cs, r)));
                break;
            default: break;  // COUNT of a no-null column = the row count
        }
    }
}

// ---- LDS-slice pipeline (k_aggregate.hip): the shapes, regions and plans its users share ----
constexpr int kSliceBits = 16;
constexpr int kSliceKeys = 1 << kSliceBits;
constexpr int kSliceMaxF = 160;                  // slices: key range <= 160 * 65536
constexpr int kSliceBlock = 1024;                // one workgroup per CU in both phases
constexpr int kSliceTile = kSliceBlock * kFastR;  // 8192 probe rows per phase-A iteration
constexpr int kSliceChunk = 32;                  // items per flushed chunk
constexpr int kMaxSliceGrid = 512;               // phase-A workgroups / build regions (items form) phase B walks
constexpr int kSliceStateWords = 3584;           // phase-B LDS aggregate states (n_slots * G)
// Group-range slices (G too large for LDS states): phase A looks the group id up and partitions
// by gid >> kGidSliceBits; phase B aggregates one range of 2^kGidSliceBits groups in LDS.
constexpr int kGidSliceBits = 12;
constexpr int kGidStateWords = 16384;            // n_slots * 2^kGidSliceBits <= this (128 KB)

struct SliceRegions {
    uint16_t *key;        // [grid][F][cap] key - kmin - slice * 2^16
    int64_t *val;         // [grid][F][cap] aggregate input (NACOL >= 1)
    int64_t *val2;        // [grid][F][cap] second aggregate input (NACOL == 2)
    uint32_t *count;      // [grid][F]
    uint32_t *overflow;   // set when a region fills up (skewed probe keys)
    uint64_t cap;         // items per region, multiple of kSliceChunk
    int32_t F;            // slices
    // exact layout (materialising join): region (workgroup r, slice b) starts at
    // rbase[b * grid + r] (slice-major, no gaps) instead of (r * F + b) * cap
    const uint64_t *rbase;
    // partitioned layout (the shuffle join's items form, pw > 0 ranks). Phase A: region (w, b) is number
    // part_region(b, w), slice-major with the slices of one destination rank (b % pw) together -- rank q's
    // regions are one contiguous block. Phase B: the packed regions received from pw ranks, local slice
    // j (global slice j * pw + prank) region (q, w) numbered (q * S + j) * pgrid + w, at rbase[number].
    int32_t pw;
    int32_t prank;
    int32_t pgrid;
    // phase B of the partitioned layout: this rank's own regions (source prank) read in place from phase
    // A's layout (region number * ocap) instead of from the packed receive buffers
    const uint16_t *okey;
    const int64_t *oval;
    uint64_t ocap;
};
// the partitioned layout's slices per rank and a region's number (phase A, pw > 0)
__host__ __device__ __forceinline__ int part_slices(int F, int pw) { return (F + pw - 1) / pw; }
__host__ __device__ __forceinline__ uint64_t part_region(int b, int w, int F, int pw, int grid) {
    return ((uint64_t)(b % pw) * part_slices(F, pw) + (uint64_t)(b / pw)) * grid + w;
}

// Phase A's shape when it is planned on the device (the prelaunch ahead of the build reads the build
// key's range from device memory instead of waiting for the host: no host round trip between the
// min/max kernels and phase A).  plan_slices is the one rule, evaluated on the device by
// k_slice_plan and on the host to adopt the result; regions are allocated for the worst case and
// the plan's cap divides them among grid x F regions.
struct SlicePlan {
    int64_t kmin;
    uint64_t range;
    uint64_t cap;
    int32_t F;
    int32_t ok;
    int64_t src[6];  // the build ranges it was planned from: key min, max, count, group key min, max, count
};
struct SlicePlanIn {
    uint64_t min_bytes;    // smallest table (bytes) worth the two-phase pipeline
    uint64_t alloc_items;  // items allocated for all regions together
    int32_t grid;
    int32_t n_slots;
    int32_t sparse_ok;     // direct_table_ok's sparse rule enabled
    int32_t chunk;         // items per flushed chunk (regions are whole chunks); 0 = kSliceChunk
    int32_t world;         // > 1: the partitioned layout's regions (F rounded up to a multiple of world)
};
__host__ __device__ inline SlicePlan plan_slices(const SlicePlanIn &pi, int64_t kmn, int64_t kmx, int64_t kcnt, int64_t gmn,
                                                 int64_t gmx, int64_t gcnt) {
    SlicePlan p{};
    p.src[0] = kmn, p.src[1] = kmx, p.src[2] = kcnt, p.src[3] = gmn, p.src[4] = gmx, p.src[5] = gcnt;
    if (kcnt <= 0) return p;
    // the group count is at most the group key's range (+ the NULL group)
    const uint64_t gr = gcnt ? (uint64_t)gmx - (uint64_t)gmn + 1ull : 0;
    const int64_t g_bound = (gr == 0 || gr > (1ull << 20)) ? -1 : (int64_t)gr + 1;
    if (g_bound <= 0 || g_bound >= 0xFFFF || (int64_t)pi.n_slots * g_bound > kSliceStateWords) return p;
    const uint64_t range = (uint64_t)kmx - (uint64_t)kmn + 1ull;
    // the DIRECT rule of build_join_table, and the slice path's own limits
    if (!direct_table_ok_with(range, (uint64_t)kcnt, (uint64_t)g_bound, pi.sparse_ok != 0)) return p;
    if (range * 2 < pi.min_bytes) return p;
    const uint64_t F = (range + kSliceKeys - 1) >> kSliceBits;
    if (F == 0 || F > (uint64_t)kSliceMaxF) return p;
    p.kmin = kmn;
    p.range = range;
    p.F = (int32_t)F;
    const uint64_t ch = pi.chunk > 0 ? (uint64_t)pi.chunk : (uint64_t)kSliceChunk;
    const uint64_t Fr = pi.world > 1 ? (F + pi.world - 1) / pi.world * pi.world : F;  // regions' slices
    p.cap = pi.alloc_items / ((uint64_t)pi.grid * Fr) / ch * ch;
    p.ok = p.cap >= ch;
    return p;
}

// The fused pipeline's plan (qeh_join_filter_aggregate with one bounded integer group key): the slice
// shape of the build key's range plus the group key's range -- the join table's entries are group
// slots (g - gmin + 1) instead of dense group ids, so the build needs no group table first.
struct FusedPlan {
    SlicePlan sp;      // sp.ok: every condition of the fused pipeline holds
    int64_t gmin;      // group slot s <-> group key gmin + s
    int64_t ngroups;   // gmax - gmin + 1
    uint64_t dcap;     // build rows per (phase-A workgroup, slice) region, a multiple of 4
};
// Phase A's prologue in the fused pipeline: the build rows grouped by slice into per-(workgroup,
// slice) regions (items = key offset << 16 | group slot + 1), and the output group keys.
struct FusedPro {
    const int64_t *dk;     // build key (Int64, no NULLs)
    ColRef dg;             // group key (Int64 / Int32, no NULLs)
    int64_t nd;
    uint32_t *ditems;      // [grid][F][dcap]
    uint32_t *dcount;      // [grid][F]
    uint32_t *status;      // [1]: a region overflowed (probe or build rows)
    void *gkeys;           // output group keys: gmin + i for i < G (Int32 when as32)
    uint32_t *rep;         // i (the finalize's representative rows)
    int64_t G;
    int32_t as32;
    const FusedPlan *plan;
};
// Phase B's view of the build rows (DIM): slice b's rows are items[(r * F + b) * dcap ..] for every
// phase-A workgroup r, count[r * F + b] of them.
struct DimSlices {
    const uint32_t *items;
    const uint32_t *count;
    uint32_t *dup;     // set when two build rows share a key
    const FusedPlan *plan;
    // the items form of the distributed broadcast join: the build rows come grouped by slice from the
    // ranks instead of from phase A's prologue -- nreg > 0 regions (every rank's build spans), region r's
    // items at items + r * rstride, with o = offs + r * 2 * (kSliceMaxF + 1): slice b's o[S + 1 + b] items
    // at o[b] (a multiple of 4)
    int32_t nreg;
    int32_t _pad;
    uint64_t rstride;
    const uint32_t *offs;
};

// Phase A's pairs per lane (P), chunk (CH) and tile by aggregate columns; EARLY (the fused pipeline) may
// take its own tile and chunk at build time (see k_slice_partition).
#ifndef QEH_EARLY_PAIRS
#define QEH_EARLY_PAIRS 2
#endif
#ifndef QEH_EARLY_CHUNK
#define QEH_EARLY_CHUNK 64
#endif
template <int NACOL, bool EARLY = false, int NTH = kSliceBlock>
struct SliceShape {
    static constexpr int P = NACOL > 1 ? 2 : (EARLY ? QEH_EARLY_PAIRS : kFastPairs);
    static constexpr int CH = NACOL > 1 ? 16 : (EARLY ? QEH_EARLY_CHUNK : kSliceChunk);
    static constexpr int TILE = NTH * 2 * P;
};

// ---- output columns of the finalize kernels (k_finalize, k_fused_finish) ----
struct OutCol {
    void *values;
    uint32_t *validity;  // nullptr when never null
    int32_t dtype;
    int32_t _pad;
};
struct OutCols {
    OutCol c[kMaxGroupKeys + kMaxAggs];
};

__device__ __forceinline__ void write_value(const OutCol &o, int64_t p, int64_t payload, bool valid) {
    if (o.validity && valid) atomicOr(&o.validity[p >> 5], 1u << (p & 31));
    switch (o.dtype) {
        case QEH_DT_BOOL:
            if (payload & 1) atomicOr(&((uint32_t *)o.values)[p >> 5], 1u << (p & 31));
            break;
        case QEH_DT_INT32: ((int32_t *)o.values)[p] = (int32_t)payload; break;
        case QEH_DT_FLOAT32: ((float *)o.values)[p] = (float)as_f64(payload); break;
        default: ((int64_t *)o.values)[p] = payload; break;  // INT64, FLOAT64 bits
    }
}

}  // namespace qeh
