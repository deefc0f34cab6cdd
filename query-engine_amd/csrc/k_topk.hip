// ORDER BY ... LIMIT k: the first k entries of the stable sort permutation without sorting the rest.
//
// The planner emits it as Limit { input: Sort } (crates/query-planner/src/planner.rs:294-303); the
// reference's execute_sort is the identity, so the semantics are those of
// qeh_sort_indices cut to `limit` rows.
//
// 1. Select (MSD radix select on the first key).  The key is encoded as sort_by_column encodes it
//    (NULL -> 0, value -> x - mn + bias ascending / mx - x + bias descending, bias = 1 when the
//    column has NULLs), `bits` significant bits.  Pass p histograms the kTkBits-wide digit p (from
//    the top) of the rows whose higher digits equal the prefix chosen so far; a one-workgroup pick
//    kernel finds the bin that holds the limit-th smallest code, extends the prefix, and keeps
//    {prefix, remaining, rows below, bin count, threshold, done} in a device struct the next pass
//    reads -- no host round trip between passes.  The walk stops once (rows below + bin count) is
//    small: the threshold T is then the chosen bin's upper bound, a superset of the candidates.
// 2. Ordered compaction.  The row ids with code <= T in ascending row order: count per workgroup
//    chunk, scan, write (chunks are contiguous row ranges, so the order is input order).
// 3. Finish.  Gather every key at the m candidates, run the full stable sort over those m rows and
//    emit cand[perm_small[i]], i < limit.
//
// Exactness: every row of the true prefix has first-key code <= T (T is at least the limit-th
// smallest code), so the prefix rows are all candidates; and a stable sort of a subsequence taken in
// input order gives those rows the relative order the full stable sort gives them (both order by
// (keys, input position)), so the first `limit` of the candidates' sort are the full sort's.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "device_common.h"
#include "ops.h"
#include "sort.h"

namespace qeh {

// 11-bit digits: a 64-bit key takes 6 passes (8 bits: 8; 12 bits: also 6, with a histogram twice the
// size), a 32-bit key 3 and anything up to 2^11 distinct codes one; the 2048-bin histogram is 8 KiB
// of LDS per workgroup and two bins per thread of the pick kernel.
constexpr int kTkBits = 11;
constexpr int kTkBins = 1 << kTkBits;
constexpr int kTkThreads = 1024;
constexpr int kTkUnroll = 4;  // 16-B loads in flight per thread

// Fallbacks to the full sort cut to `limit`, each set from the sweep in DESIGN.md §5 "Top-k": fewer
// than kTkMinRows rows (QEH_TOPK_MIN_ROWS overrides per call), limit >= n / kTkLimitShare, m >= n /
// kTkCandShare candidates (mass ties at the threshold), or one key of at most kTkOnePassBits bits
// (the full sort is then a single radix pass, which the select's passes do not beat).
constexpr int64_t kTkMinRows = 1 << 22;
constexpr int64_t kTkLimitShare = 16;
constexpr int64_t kTkCandShare = 16;
constexpr int kTkOnePassBits = 7;
// the select stops refining once the candidates fit this many rows beyond `limit`
constexpr int64_t kTkStopRows = 1 << 16;

struct TkState {
    uint64_t prefix;     // the digits chosen so far = the high bits of the threshold
    uint64_t remaining;  // rank (1-based) of the wanted code among the rows of the chosen bin
    uint64_t below;      // rows whose code is below the chosen bin
    uint64_t bin_count;  // rows in the chosen bin
    uint64_t thresh;     // the chosen bin's upper bound: candidates are the rows with code <= thresh
    uint64_t m;          // candidates = below + bin_count of the last pass that ran
    uint32_t done;       // later passes return at once
    uint32_t passes;     // passes that ran
};

// The first key as the kernels read it: `base` is the values pointer moved back by `pad` elements
// to a 16-B boundary, so group g is the 16 bytes at base + 16 g = rows [g V - pad, g V - pad + V).
struct TkKey {
    const char *base;
    const uint8_t *validity;  // nullptr: no NULLs
    int64_t vbit0;
    int64_t n, pad;
    int64_t mn, mx;
    uint64_t bias;
    int32_t dtype, asc;
};

typedef unsigned int tk_u32x4 __attribute__((ext_vector_type(4)));

// the 16 bytes of group g (rows outside [0, n) read as 0: the edge groups load row by row, a group
// past the end nothing)
template <int ES>
__device__ __forceinline__ tk_u32x4 tk_load(const TkKey &k, int64_t g) {
    constexpr int V = 16 / ES;
    const int64_t r0 = g * V - k.pad;
    if (r0 >= 0 && r0 + V <= k.n) return __builtin_nontemporal_load((const tk_u32x4 *)k.base + g);
    tk_u32x4 q = {0u, 0u, 0u, 0u};
    const uint32_t *w = (const uint32_t *)k.base + g * 4;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        if (r0 + v < 0 || r0 + v >= k.n) continue;
        if constexpr (ES == 4) {
            q[v] = w[v];
        } else {
            q[2 * v] = w[2 * v];
            q[2 * v + 1] = w[2 * v + 1];
        }
    }
    return q;
}

// codes of group g's rows; bit v of the result = row v is inside [0, n)
template <int ES>
__device__ __forceinline__ uint32_t tk_codes(const TkKey &k, const tk_u32x4 &q, int64_t g, uint64_t *code) {
    constexpr int V = 16 / ES;
    const int64_t r0 = g * V - k.pad;
    uint32_t live = 0;
#pragma unroll
    for (int v = 0; v < V; ++v) {
        const int64_t row = r0 + v;
        const bool in = row >= 0 && row < k.n;
        int64_t x;
        if constexpr (ES == 4) {
            const uint32_t w = q[v];
            if (k.dtype == QEH_DT_FLOAT32) x = f64_order_key((double)__builtin_bit_cast(float, w));
            else if (k.dtype == QEH_DT_UINT32) x = (int64_t)w;
            else x = (int64_t)(int32_t)w;
        } else {
            const int64_t w = (int64_t)((uint64_t)q[2 * v] | ((uint64_t)q[2 * v + 1] << 32));
            x = k.dtype == QEH_DT_FLOAT64 ? f64_order_key(__builtin_bit_cast(double, w)) : w;
        }
        const uint64_t c = k.asc ? (uint64_t)x - (uint64_t)k.mn + k.bias : (uint64_t)k.mx - (uint64_t)x + k.bias;
        const bool valid = !k.validity || (in && bit_at(k.validity, k.vbit0 + row));
        code[v] = valid ? c : 0;
        live |= in ? 1u << v : 0u;
    }
    return live;
}

// lanes of this wave whose digit equals mine (radix_device.h's digit_peers at this digit width)
__device__ __forceinline__ uint64_t tk_peers(uint32_t dg, bool live) {
    uint64_t peers = __ballot(live);
#pragma unroll
    for (int b = 0; b < kTkBits; ++b) {
        const uint64_t m = __ballot((dg >> b) & 1);
        peers &= ((dg >> b) & 1) ? m : ~m;
    }
    return peers;
}

// One row per lane into the workgroup's LDS histogram.  Equal digits are summed inside the wave
// first: a wave whose live lanes all share one digit (a low-cardinality key, or the rows of one
// narrow bin) adds once; a wave where the first live lane's digit still fills an eighth of the lanes
// adds once per distinct digit; the rest (spread digits) add one per lane, which collide rarely.
__device__ __forceinline__ void tk_hist_add(uint32_t *h, uint32_t dg, bool live) {
    const uint64_t lm = __ballot(live);
    if (lm == 0) return;
    const uint32_t d0 = (uint32_t)__shfl((int)dg, __ffsll((unsigned long long)lm) - 1, 64);
    const uint64_t same = __ballot(live && dg == d0);
    if (same == lm) {
        if (live && mbcnt(lm) == 0) atomicAdd(&h[d0], (uint32_t)popc64(lm));
    } else if (popc64(same) >= 8) {
        const uint64_t peers = tk_peers(dg, live);
        if (live && mbcnt(peers) == 0) atomicAdd(&h[dg], (uint32_t)popc64(peers));
    } else if (live) {
        atomicAdd(&h[dg], 1u);
    }
}

// Pass of the select: digit (code >> shift) & mask of every row with code >> hi_shift == prefix
// (first pass: every row) into ghist; mask = the pass's digit width (the last pass may be narrower).
// Grid-stride over 16-B groups, kTkUnroll loads in
// flight per thread; the loop bounds are workgroup-uniform (the wave helpers need every lane).
template <int ES>
__global__ __launch_bounds__(kTkThreads) void k_topk_hist(TkKey k, int64_t ngroups, int first, int hi_shift, int shift,
                                                          uint32_t mask, const TkState *__restrict__ st, uint32_t *__restrict__ ghist) {
    constexpr int V = 16 / ES;
    __shared__ uint32_t h[kTkBins];
    if (st->done) return;
    const uint64_t prefix = st->prefix;
    for (int i = threadIdx.x; i < kTkBins; i += kTkThreads) h[i] = 0;
    __syncthreads();
    const int64_t stride = (int64_t)gridDim.x * kTkThreads;
    for (int64_t gb = (int64_t)blockIdx.x * kTkThreads; gb < ngroups; gb += kTkUnroll * stride) {
        tk_u32x4 q[kTkUnroll];
#pragma unroll
        for (int u = 0; u < kTkUnroll; ++u) {
            const int64_t g = gb + u * stride + threadIdx.x;
            q[u] = g < ngroups ? tk_load<ES>(k, g) : tk_u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int u = 0; u < kTkUnroll; ++u) {
            const int64_t g = gb + u * stride + threadIdx.x;
            uint64_t code[V];
            const uint32_t live = tk_codes<ES>(k, q[u], g, code);  // (a group past the end has no live row)
#pragma unroll
            for (int v = 0; v < V; ++v) {
                const bool take = ((live >> v) & 1) && (first || (code[v] >> hi_shift) == prefix);
                tk_hist_add(h, (uint32_t)(code[v] >> shift) & mask, take);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < kTkBins; i += kTkThreads)
        if (h[i]) atomicAdd(&ghist[i], h[i]);
}

// One workgroup: the bin that holds the remaining-th smallest row of this pass, the new state, and
// the histogram cleared for the next pass.  `width` = bits of this pass's digit, `last` = no digits
// below it, stop_at: candidates (rows below + bin) at which the walk stops early.
__global__ __launch_bounds__(kTkThreads) void k_topk_pick(uint32_t *__restrict__ ghist, TkState *__restrict__ st, int shift,
                                                          int width, int last, uint64_t stop_at) {
    static_assert(kTkBins == 2 * kTkThreads, "two bins per thread");
    __shared__ uint32_t wsum[kTkThreads / 64];
    const TkState s = *st;
    if (s.done) return;  // (the histogram is clear: the pass that set `done` cleared it)
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const uint32_t c0 = ghist[2 * t], c1 = ghist[2 * t + 1];
    ghist[2 * t] = 0;
    ghist[2 * t + 1] = 0;
    // (bin totals sum to at most n < 2^32)
    const uint32_t sum = c0 + c1, incl = wave_incl_scan(sum);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();  // also orders every thread's read of *st before the owner's write below
    uint64_t excl = incl - sum;
    for (int w = 0; w < wave; ++w) excl += wsum[w];
    if (excl < s.remaining && s.remaining <= excl + sum) {  // exactly one thread: the bins hold >= remaining rows
        const bool lo = s.remaining <= excl + c0;
        const uint64_t d = 2 * t + (lo ? 0 : 1), before = excl + (lo ? 0 : c0), cnt = lo ? c0 : c1;
        TkState o = s;
        o.prefix = (width >= 64 ? 0 : s.prefix << width) | d;
        o.below = s.below + before;
        o.remaining = s.remaining - before;
        o.bin_count = cnt;
        o.thresh = ((o.prefix + 1) << shift) - 1;  // (wraps to all ones at the top of a 64-bit code)
        o.done = (last || o.below + cnt <= stop_at) ? 1u : 0u;
        o.m = o.below + cnt;
        o.passes = s.passes + 1;
        *st = o;
    }
}

// rows of chunk b (groups [b gseg, (b + 1) gseg)) with code <= thresh -> cnt[b]
template <int ES>
__global__ __launch_bounds__(kTkThreads) void k_topk_count(TkKey k, int64_t ngroups, int64_t gseg,
                                                           const TkState *__restrict__ st, uint32_t *__restrict__ cnt,
                                                           uint64_t cap) {
    constexpr int V = 16 / ES;
    __shared__ uint32_t wsum[kTkThreads / 64];
    if (st->m > cap) return;  // mass ties: the caller falls back, nothing is compacted
    const uint64_t T = st->thresh;
    const int64_t lo = (int64_t)blockIdx.x * gseg, hi = lo + gseg < ngroups ? lo + gseg : ngroups;
    uint32_t acc = 0;
    for (int64_t gb = lo; gb < hi; gb += kTkUnroll * kTkThreads) {
        tk_u32x4 q[kTkUnroll];
#pragma unroll
        for (int u = 0; u < kTkUnroll; ++u) {
            const int64_t g = gb + u * kTkThreads + threadIdx.x;
            q[u] = g < hi ? tk_load<ES>(k, g) : tk_u32x4{0u, 0u, 0u, 0u};
        }
#pragma unroll
        for (int u = 0; u < kTkUnroll; ++u) {
            const int64_t g = gb + u * kTkThreads + threadIdx.x;
            uint64_t code[V];
            const uint32_t live = g < hi ? tk_codes<ES>(k, q[u], g, code) : 0u;
#pragma unroll
            for (int v = 0; v < V; ++v) acc += (((live >> v) & 1) && code[v] <= T) ? 1u : 0u;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint32_t c = 0;
        for (int w = 0; w < kTkThreads / 64; ++w) c += wsum[w];
        cnt[blockIdx.x] = c;
    }
}

// one workgroup: offs = exclusive scan of the nb <= kTkThreads chunk counts (their sum is st->m)
__global__ __launch_bounds__(kTkThreads) void k_topk_scan(const uint32_t *__restrict__ cnt, int nb, uint64_t *__restrict__ offs,
                                                          const TkState *__restrict__ st, uint64_t cap) {
    __shared__ uint32_t wsum[kTkThreads / 64];
    if (st->m > cap) return;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    const uint32_t c = t < nb ? cnt[t] : 0u, incl = wave_incl_scan(c);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint64_t excl = incl - c;
    for (int w = 0; w < wave; ++w) excl += wsum[w];
    if (t < nb) offs[t] = excl;
}

// the row ids of chunk b's candidates, in row order, at cand[offs[b]...) (more than cap candidates:
// nothing is written, the caller falls back).  A tile is kTkUnroll x kTkThreads groups in (u, thread, v)
// row order; tiles without a candidate -- nearly all of them -- skip the ranking.
template <int ES>
__global__ __launch_bounds__(kTkThreads) void k_topk_write(TkKey k, int64_t ngroups, int64_t gseg,
                                                           const TkState *__restrict__ st, const uint64_t *__restrict__ offs,
                                                           uint32_t *__restrict__ cand, uint64_t cap) {
    constexpr int V = 16 / ES;
    constexpr int W = kTkThreads / 64;
    __shared__ uint32_t wcnt[kTkUnroll][W];
    __shared__ uint32_t s_total;
    if (st->m > cap) return;
    const uint64_t T = st->thresh;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t lo = (int64_t)blockIdx.x * gseg, hi = lo + gseg < ngroups ? lo + gseg : ngroups;
    uint64_t pos0 = offs[blockIdx.x];
    for (int64_t gb = lo; gb < hi; gb += kTkUnroll * kTkThreads) {
        tk_u32x4 q[kTkUnroll];
#pragma unroll
        for (int u = 0; u < kTkUnroll; ++u) {
            const int64_t g = gb + u * kTkThreads + threadIdx.x;
            q[u] = g < hi ? tk_load<ES>(k, g) : tk_u32x4{0u, 0u, 0u, 0u};
        }
        uint32_t sel[kTkUnroll];
        uint32_t any = 0;
#pragma unroll
        for (int u = 0; u < kTkUnroll; ++u) {
            const int64_t g = gb + u * kTkThreads + threadIdx.x;
            uint64_t code[V];
            const uint32_t live = g < hi ? tk_codes<ES>(k, q[u], g, code) : 0u;
            sel[u] = 0;
#pragma unroll
            for (int v = 0; v < V; ++v) sel[u] |= (((live >> v) & 1) && code[v] <= T) ? 1u << v : 0u;
            any |= sel[u];
        }
        if (!__syncthreads_or((int)any)) continue;  // (also keeps the previous tile's LDS reads ahead of the writes below)
        uint32_t before[kTkUnroll];                 // candidates of this wave's lower lanes, per u
#pragma unroll
        for (int u = 0; u < kTkUnroll; ++u) {
            const uint32_t c = (uint32_t)__popc(sel[u]), incl = wave_incl_scan(c);
            before[u] = incl - c;
            if (lane == 63) wcnt[u][wave] = incl;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            uint32_t acc = 0;
            for (int u = 0; u < kTkUnroll; ++u)
                for (int w = 0; w < W; ++w) {
                    const uint32_t c = wcnt[u][w];
                    wcnt[u][w] = acc;
                    acc += c;
                }
            s_total = acc;
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < kTkUnroll; ++u) {
            const int64_t g = gb + u * kTkThreads + threadIdx.x;
            uint64_t p = pos0 + wcnt[u][wave] + before[u];
#pragma unroll
            for (int v = 0; v < V; ++v) {
                if (!((sel[u] >> v) & 1)) continue;
                if (p < cap) cand[p] = (uint32_t)(g * V - k.pad + v);
                ++p;
            }
        }
        pos0 += s_total;
    }
}

static int64_t topk_min_rows() {
    const char *e = std::getenv("QEH_TOPK_MIN_ROWS");
    if (!e || !*e) return kTkMinRows;
    char *end = nullptr;
    const long long v = std::strtoll(e, &end, 10);
    return (end && end != e && v >= 0) ? (int64_t)v : kTkMinRows;
}

constexpr int kTopkFallback = -4;

// The candidates of the first `limit` rows by keys[0]: *m row ids in row order in `cand`, or
// kTopkFallback when the full sort is the better (or only) way.
static int topk_select(qeh_ctx *ctx, const qeh_column &key, bool asc, bool one_key, int64_t n, int64_t limit, DevBuf *cand,
                       int64_t *m) {
    // (QEH_TOPK_FORCE: the measurement sweep's switch -- the select path at any limit and row count)
    const bool force = std::getenv("QEH_TOPK_FORCE") != nullptr;
    if (!force && (n < topk_min_rows() || limit >= n / kTkLimitShare)) return kTopkFallback;
    const size_t es = dtype_size(key.dtype);
    if (es != 4 && es != 8) return kTopkFallback;  // BOOL keys: the full sort
    int64_t mn, mx;
    QEH_TRY(sort_key_range(ctx, key, &mn, &mx));
    if (mn > mx) return kTopkFallback;  // every row NULL
    const bool nullable = key.validity != nullptr && key.null_count != 0;
    const uint64_t span = (uint64_t)mx - (uint64_t)mn;
    if (nullable && span == UINT64_MAX) return kTopkFallback;  // 2^64 values and NULL: 65 bits
    const uint64_t top = span + (nullable ? 1 : 0);
    int bits = 0;
    while (bits < 64 && (top >> bits) != 0) ++bits;
    if (bits == 0) return kTopkFallback;  // one value, no NULLs: every row ties
    if (!force && one_key && bits <= kTkOnePassBits) return kTopkFallback;

    const ColRef c = make_colref(key);
    TkKey k{};
    k.pad = (int64_t)(((uintptr_t)c.values & 15) / es);
    if (((uintptr_t)c.values & (es - 1)) != 0) return kTopkFallback;  // values not element-aligned
    k.base = (const char *)c.values - k.pad * (int64_t)es;
    k.validity = nullable ? c.validity : nullptr;
    k.vbit0 = c.vbit0;
    k.n = n;
    k.mn = mn, k.mx = mx;
    k.bias = nullable ? 1 : 0;
    k.dtype = key.dtype;
    k.asc = asc ? 1 : 0;
    const int V = (int)(16 / es);
    const int64_t ngroups = (n + k.pad + V - 1) / V;

    // candidates beyond this many mean mass ties at the threshold: the full sort
    const int64_t cap = force ? n : n / kTkCandShare;
    const int nb = grid_for(ctx, ngroups, kTkThreads * kTkUnroll, 2);  // <= kTkThreads chunks (k_topk_scan)
    if (nb > kTkThreads) return kTopkFallback;
    const int64_t gseg = (ngroups + nb - 1) / nb;
    DevBuf state, hist, cnt, offs;
    QEH_TRY(state.alloc(ctx, sizeof(TkState)));
    QEH_TRY(hist.alloc(ctx, kTkBins * 4));
    QEH_TRY(cnt.alloc(ctx, (size_t)nb * 4));
    QEH_TRY(offs.alloc(ctx, (size_t)nb * 8));
    QEH_TRY(cand->alloc(ctx, (size_t)cap * 4));
    TkState init{};
    init.remaining = (uint64_t)limit;
    init.thresh = UINT64_MAX;
    QEH_HIP(hipMemcpyAsync(state.p, &init, sizeof init, hipMemcpyHostToDevice, ctx->stream));
    QEH_HIP(hipMemsetAsync(hist.p, 0, kTkBins * 4, ctx->stream));
    TkState *st = state.as<TkState>();
    {
        KernelTimer kt(ctx, "topk_select");
        const int passes = (bits + kTkBits - 1) / kTkBits;
        const uint64_t stop_at = (uint64_t)std::min<int64_t>(limit + kTkStopRows, cap);
        for (int p = 0; p < passes; ++p) {
            const int hi_shift = bits - kTkBits * p, shift = std::max(hi_shift - kTkBits, 0);
            const uint32_t mask = (1u << (hi_shift - shift)) - 1u;
            if (es == 4)
                hipLaunchKernelGGL(k_topk_hist<4>, dim3(nb), dim3(kTkThreads), 0, ctx->stream, k, ngroups, p == 0 ? 1 : 0,
                                   hi_shift & 63, shift, mask, st, hist.as<uint32_t>());
            else
                hipLaunchKernelGGL(k_topk_hist<8>, dim3(nb), dim3(kTkThreads), 0, ctx->stream, k, ngroups, p == 0 ? 1 : 0,
                                   hi_shift & 63, shift, mask, st, hist.as<uint32_t>());
            hipLaunchKernelGGL(k_topk_pick, dim3(1), dim3(kTkThreads), 0, ctx->stream, hist.as<uint32_t>(), st, shift,
                               hi_shift - shift, p == passes - 1 ? 1 : 0, stop_at);
        }
        if (es == 4)
            hipLaunchKernelGGL(k_topk_count<4>, dim3(nb), dim3(kTkThreads), 0, ctx->stream, k, ngroups, gseg, st,
                               cnt.as<uint32_t>(), (uint64_t)cap);
        else
            hipLaunchKernelGGL(k_topk_count<8>, dim3(nb), dim3(kTkThreads), 0, ctx->stream, k, ngroups, gseg, st,
                               cnt.as<uint32_t>(), (uint64_t)cap);
        hipLaunchKernelGGL(k_topk_scan, dim3(1), dim3(kTkThreads), 0, ctx->stream, cnt.as<uint32_t>(), nb, offs.as<uint64_t>(), st,
                           (uint64_t)cap);
        if (es == 4)
            hipLaunchKernelGGL(k_topk_write<4>, dim3(nb), dim3(kTkThreads), 0, ctx->stream, k, ngroups, gseg, st,
                               offs.as<uint64_t>(), cand->as<uint32_t>(), (uint64_t)cap);
        else
            hipLaunchKernelGGL(k_topk_write<8>, dim3(nb), dim3(kTkThreads), 0, ctx->stream, k, ngroups, gseg, st,
                               offs.as<uint64_t>(), cand->as<uint32_t>(), (uint64_t)cap);
    }
    QEH_HIP(hipGetLastError());
    TkState fin{};
    QEH_TRY(read_small(ctx, &fin, state.p, sizeof fin));
    if (fin.m < (uint64_t)limit) return fail(QEH_E_INTERNAL, "top-k select found fewer candidates than the limit");
    if (fin.m > (uint64_t)cap) return kTopkFallback;
    *m = (int64_t)fin.m;
    return QEH_OK;
}

}  // namespace qeh

using namespace qeh;

extern "C" int qeh_sort_indices_limit(qeh_ctx *ctx, const qeh_column *keys, int n_keys, const int8_t *ascending,
                                      int64_t limit, qeh_column *out_perm) {
    if (!ctx || !keys || !out_perm) return fail(QEH_E_INVALID, "qeh_sort_indices_limit: bad argument");
    if (limit < 0) return fail(QEH_E_INVALID, "qeh_sort_indices_limit: negative limit");
    DeviceGuard dg(ctx->device);
    if (any_recoded_key(keys, n_keys)) {  // codes compare as the strings do; temporal keys as their integers
        Utf8Keys uk;
        QEH_TRY(encode_utf8_keys(ctx, keys, n_keys, &uk));
        return qeh_sort_indices_limit(ctx, uk.keys.data(), n_keys, ascending, limit, out_perm);
    }
    int64_t n;
    QEH_TRY(check_sort_keys(keys, n_keys, &n));
    if (limit == 0 || n == 0) {
        QEH_TRY(alloc_column(ctx, QEH_DT_UINT32, 0, false, out_perm));
        return QEH_OK;
    }
    if (limit < n && !std::getenv("QEH_NO_TOPK")) {
        DevBuf cand;
        int64_t m = 0;
        const int s = topk_select(ctx, keys[0], ascending ? ascending[0] != 0 : true, n_keys == 1, n, limit, &cand, &m);
        if (s == QEH_OK) {
            std::vector<qeh_column> sub(n_keys);
            int g = QEH_OK;
            int made = 0;
            for (; made < n_keys && g == QEH_OK; ++made) g = gather_column(ctx, keys[made], cand.as<uint32_t>(), m, &sub[made]);
            if (g != QEH_OK) --made;  // (the failed gather allocated nothing it kept)
            if (g == QEH_OK) g = sort_perm_prefix(ctx, sub.data(), n_keys, ascending, m, limit, cand.as<uint32_t>(), out_perm);
            else (void)hipStreamSynchronize(ctx->stream);
            for (int j = 0; j < made; ++j) qeh_column_release(ctx, &sub[j]);
            return g;
        }
        if (s != kTopkFallback) return s;
    }
    return sort_perm_prefix(ctx, keys, n_keys, ascending, n, limit, nullptr, out_perm);
}
