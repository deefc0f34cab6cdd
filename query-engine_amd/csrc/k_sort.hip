// SortExec: LSD radix sort with LDS histograms producing a stable permutation, and the
// payload-carrying sort behind Merge::sorted.  What other units use of it is declared in sort.h.
//
// Reference: execute_sort is the identity (crates/query-executor/src/executor.rs:290-297),
// so the semantics are the intended ones of SURVEY.md §8.0: stable lexicographic sort
// by `exprs` with a per-key ascending flag, NULLs first (arrow SortOptions
// default; the only explicit null ordering in the tree is
// distributed/operators.rs:97-104), floats by totalOrder.
//
// Key encoding: each key column becomes an unsigned integer in [0, 2^bits):
// NULL -> 0, value -> (ordered(x) - min + 1) ascending or (max - ordered(x) + 1)
// descending, where ordered() is sign-flip for ints and totalOrder for floats
// and min/max come from one reduction.  Only `bits` = bit length of the range
// are sorted (e.g. 21 bits for k in [0, 2^20)), 8 bits per pass; keys are
// processed last column first, each column's passes reading its encoding
// through the current permutation, so the result is lexicographic and stable.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "radix_device.h"
#include "sort.h"

namespace qeh {

struct KeyStats {
    int64_t mn, mx;
};

constexpr int kRsMaxSegs = 16;  // Merge::sorted partitions read in place (RsEncode, KeySegs)

// (block bid of nb over the rows: k_key_stats runs it for one column, k_key_stats_segs for one segment each)
__device__ __forceinline__ void key_stats_body(const ColRef &c, const uint32_t *__restrict__ perm, int64_t n, KeyStats *out,
                                               int64_t bid, int64_t nb) {
    int64_t mn = INT64_MAX, mx = INT64_MIN;
    if (!perm && !c.validity && c.dtype == QEH_DT_INT64 && ((uintptr_t)c.values & 15) == 0) {
        // plain int64 column: 16-B loads, four in flight per thread
        typedef long long v2 __attribute__((ext_vector_type(2)));
        const v2 *kv = (const v2 *)c.values;
        const int64_t pairs = n / 2, stride = nb * blockDim.x;
        for (int64_t i = bid * blockDim.x + threadIdx.x; i < pairs; i += 4 * stride) {
            v2 q[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) q[u] = kv[i + u * stride < pairs ? i + u * stride : i];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                mn = q[u].x < mn ? q[u].x : mn;
                mx = q[u].x > mx ? q[u].x : mx;
                mn = q[u].y < mn ? q[u].y : mn;
                mx = q[u].y > mx ? q[u].y : mx;
            }
        }
        if ((n & 1) && bid == 0 && threadIdx.x == 0) {
            const int64_t k = ((const int64_t *)c.values)[n - 1];
            mn = k < mn ? k : mn;
            mx = k > mx ? k : mx;
        }
    } else if (!perm && c.dtype == QEH_DT_INT64 && (c.vbit0 & 7) == 0 && ((uintptr_t)c.values & 15) == 0) {
        // nullable int64 column whose validity bytes line up with the rows: eight rows per thread
        // (one validity byte, four 16-B loads), rows of NULLs skipped by mask
        typedef long long v2 __attribute__((ext_vector_type(2)));
        const uint8_t *vb = c.validity + (c.vbit0 >> 3);
        // (four groups per iteration: 16 loads in flight per thread, the grid is one workgroup per CU)
        const int64_t groups = n / 8, stride = nb * blockDim.x;
        for (int64_t g0 = bid * blockDim.x + threadIdx.x; g0 < groups; g0 += 4 * stride) {
            uint32_t m[4];
            v2 q[4][4];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const int64_t g = g0 + w * stride < groups ? g0 + w * stride : g0;
                m[w] = g0 + w * stride < groups ? vb[g] : 0u;  // (a clamped repeat counts nothing)
                const v2 *kv = (const v2 *)c.values + g * 4;
#pragma unroll
                for (int u = 0; u < 4; ++u) q[w][u] = kv[u];
            }
#pragma unroll
            for (int w = 0; w < 4; ++w)
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    if ((m[w] >> (2 * u)) & 1u) mn = q[w][u].x < mn ? q[w][u].x : mn, mx = q[w][u].x > mx ? q[w][u].x : mx;
                    if ((m[w] >> (2 * u + 1)) & 1u) mn = q[w][u].y < mn ? q[w][u].y : mn, mx = q[w][u].y > mx ? q[w][u].y : mx;
                }
        }
        for (int64_t i = groups * 8 + bid * blockDim.x + threadIdx.x; i < n; i += stride) {
            if (!col_valid(c, i)) continue;
            const int64_t k = ((const int64_t *)c.values)[i];
            mn = k < mn ? k : mn;
            mx = k > mx ? k : mx;
        }
    } else {
        for (int64_t i = bid * blockDim.x + threadIdx.x; i < n; i += nb * blockDim.x) {
            const int64_t r = perm ? perm[i] : i;
            if (!col_valid(c, r)) continue;
            const int64_t k = ordered_key(c, r);
            mn = k < mn ? k : mn;
            mx = k > mx ? k : mx;
        }
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const int64_t a = __shfl_xor(mn, d, 64), b = __shfl_xor(mx, d, 64);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if ((threadIdx.x & 63) == 0) {
        atomicMin((long long *)&out->mn, (long long)mn);
        atomicMax((long long *)&out->mx, (long long)mx);
    }
}

__global__ void k_key_stats(ColRef c, const uint32_t *__restrict__ perm, int64_t n, KeyStats *out) {
    key_stats_body(c, perm, n, out, blockIdx.x, gridDim.x);
}

// one launch over up to kRsMaxSegs columns (Merge::sorted's partitions): gps blocks per segment
struct KeySegs {
    int32_t ns, gps;
    ColRef c[kRsMaxSegs];
    int64_t n[kRsMaxSegs];
};
__global__ void k_key_stats_segs(KeySegs ks, KeyStats *out) {
    const int seg = blockIdx.x / ks.gps;
    key_stats_body(ks.c[seg], nullptr, ks.n[seg], out, blockIdx.x % ks.gps, ks.gps);
}

__global__ void k_stats_init(KeyStats *s) {
    s->mn = INT64_MAX;
    s->mx = INT64_MIN;
}

// encoded key of row perm[i] (or i) -> keys[i]; perm_out[i] = perm[i] (or i)
// mode 0: value encoding (NULL -> 0, values biased by `bias`); mode 1: null flag only
// `null_code`: the key of a NULL row (0 = NULLs first; above every value code = NULLs last)
template <typename KeyT>
__global__ void k_encode(ColRef c, const uint32_t *__restrict__ perm, int64_t n, int64_t mn, int64_t mx, int asc,
                         uint64_t bias, int mode, uint64_t null_code, KeyT *__restrict__ keys,
                         uint32_t *__restrict__ perm_out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = perm ? perm[i] : i;
        uint64_t k = null_code;
        if (col_valid(c, r)) {
            if (mode == 1) {
                k = null_code ? 0 : 1;
            } else {
                const int64_t x = ordered_key(c, r);
                k = asc ? (uint64_t)x - (uint64_t)mn + bias : (uint64_t)mx - (uint64_t)x + bias;
            }
        }
        keys[i] = (KeyT)k;
        perm_out[i] = (uint32_t)r;
    }
}

// ---- one LSD pass ----------------------------------------------------------------------
// Block b owns elements [b*seg, (b+1)*seg) and walks them in tiles of kRsTile;
// inside a tile wave w owns the contiguous run [w*64*kRsIpt, (w+1)*64*kRsIpt)
// and its item j is element w*64*kRsIpt + j*64 + lane, so (wave, j, lane) is
// input order and every load is a full 512-byte wave line.  hist is digit-major
// [kRadix][nblocks].  The tile constants and the in-tile ranking are in radix_device.h.

// The payload sort's first pass reads the raw key column and encodes on load (KES = 4 / 8: Int32 /
// Int64 values) instead of a separate encode pass; KES = 0 reads the codes.
// ns > 0: the first pass reads the key and payload in place from ns row segments (qeh_merge_sorted's
// partitions: rows [start[s], start[s + 1]) are segment s's rows 0..) instead of one column -- no
// concatenation copy ahead of the sort (kRsMaxSegs: at the top of the file)
struct RsEncode {
    ColRef c;
    int64_t mn, mx;
    uint64_t bias, null_code;
    int32_t asc;
    int32_t ns;
    int64_t start[kRsMaxSegs + 1];
    ColRef sk[kRsMaxSegs];
    const uint64_t *sv[kRsMaxSegs];
    // KES = 1 (the MSD payload sort's second pass): the keys are the low 32 code bits, and the byte
    // stream nd holds code bits [nd_shift, nd_shift + 8) -- all the pass reads of a code
    const uint8_t *nd;
    int32_t nd_shift;
};

// the segment of row i (branch-free count of the segment starts at or below i)
__device__ __forceinline__ int rs_seg(const RsEncode &e, int64_t i) {
    int s = 0;
#pragma unroll
    for (int q = 1; q < kRsMaxSegs; ++q) s += (q < e.ns && i >= e.start[q]) ? 1 : 0;
    return s;
}

// the segment of a tile's rows [a, b] when they share one (wave-uniform: a scalar index into the kernel
// arguments), else -1 (rows straddle a partition boundary: looked up per row)
__device__ __forceinline__ int rs_tile_seg(const RsEncode &e, int64_t a, int64_t b) {
    if (!e.ns) return 0;
    const int sa = rs_seg(e, a), sb = rs_seg(e, b);
    return __builtin_amdgcn_readfirstlane(sa == sb ? sa : -1);
}

template <int KES>
__device__ __forceinline__ uint64_t rs_code(const RsEncode &e, const ColRef &c, int64_t i) {
    const int64_t x = KES == 4 ? (int64_t)__builtin_nontemporal_load((const int32_t *)c.values + i)
                               : __builtin_nontemporal_load((const int64_t *)c.values + i);
    const uint64_t code = e.asc ? (uint64_t)x - (uint64_t)e.mn + e.bias : (uint64_t)e.mx - (uint64_t)x + e.bias;
    return col_valid(c, i) ? code : e.null_code;
}

// (segments are only ever indexed by a wave-uniform value: a per-lane index into the kernel arguments
// would copy the whole RsEncode to scratch)
template <int KES, typename KeyT>
__device__ __forceinline__ KeyT rs_load_key(const KeyT *__restrict__ keys, const RsEncode &e, int64_t i, int ts = 0) {
    if constexpr (KES == 0) {
        return __builtin_nontemporal_load(&keys[i]);
    } else if constexpr (KES == 1) {
        const uint32_t lo = __builtin_nontemporal_load((const uint32_t *)keys + i);
        return ((KeyT)e.nd[i] << e.nd_shift) | (KeyT)(lo & ((1u << e.nd_shift) - 1u));
    } else {
        if (!e.ns) return (KeyT)rs_code<KES>(e, e.c, i);
        if (ts >= 0) return (KeyT)rs_code<KES>(e, e.sk[ts], i - e.start[ts]);
        uint64_t code = 0;
        for (int s = 0; s < e.ns; ++s)  // (a tile across a partition boundary)
            if (i >= e.start[s] && i < e.start[s + 1]) code = rs_code<KES>(e, e.sk[s], i - e.start[s]);
        return (KeyT)code;
    }
}

// the first pass's payload of row i (in place from the segments when ns > 0)
template <int KES, typename ValT>
__device__ __forceinline__ ValT rs_load_val(const ValT *__restrict__ vals, const RsEncode &e, int64_t i, int ts = 0) {
    if constexpr (KES >= 4 && sizeof(ValT) == 8) {
        if (e.ns) {
            if (ts >= 0) return (ValT)__builtin_nontemporal_load(e.sv[ts] + (i - e.start[ts]));
            ValT v = 0;
            for (int s = 0; s < e.ns; ++s)
                if (i >= e.start[s] && i < e.start[s + 1]) v = (ValT)__builtin_nontemporal_load(e.sv[s] + (i - e.start[s]));
            return v;
        }
    }
    return __builtin_nontemporal_load(&vals[i]);
}

template <typename KeyT, int KES = 0>
__global__ __launch_bounds__(kRsThreads) void k_rs_hist(const KeyT *__restrict__ keys, int64_t n, int64_t seg,
                                                        int shift, uint32_t *__restrict__ hist, int nblocks, RsEncode enc) {
    constexpr int W = kRsThreads / 64;
    __shared__ uint32_t h[W][kRadix];  // per-wave counters: one LDS atomic per row
    for (int i = threadIdx.x; i < W * kRadix; i += kRsThreads) (&h[0][0])[i] = 0;
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * seg, hi = lo + seg < n ? lo + seg : n;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (int64_t c0 = lo; c0 < hi; c0 += kRsSTile) {
        const int64_t base = c0 + (int64_t)wave * 64 * kRsIpt + lane;
        const int ts = KES != 0 ? rs_tile_seg(enc, c0, (c0 + kRsSTile < hi ? c0 + kRsSTile : hi) - 1) : 0;
        KeyT k[kRsIpt];
#pragma unroll
        for (int j = 0; j < kRsIpt; ++j) {
            const int64_t i = base + j * 64;
            k[j] = rs_load_key<KES>(keys, enc, i < hi ? i : hi - 1, ts);
        }
#pragma unroll
        for (int j = 0; j < kRsIpt; ++j) {
            const bool live = base + j * 64 < hi;
            const uint32_t dg = (uint32_t)((k[j] >> shift) & (kRadix - 1));
            if (live) atomicAdd(&h[wave][dg], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < kRadix) {
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) c += h[w][threadIdx.x];
        hist[(int64_t)threadIdx.x * nblocks + blockIdx.x] = c;
    }
}

// The payload sort's first histogram (KES = 8 / 4: Int64 / Int32 keys, encoded as rs_code does): a
// lane reads 8 consecutive rows of a partition with 16-B loads and their validity byte at once (row
// order does not matter to a histogram), four such groups in flight; a segment's head and tail rows,
// and columns whose values or validity do not line up, one row at a time.  Same block row ranges
// [b * seg, (b + 1) * seg) and hist layout as k_rs_hist<KeyT, KES>.
template <int KES>
__global__ __launch_bounds__(kRsThreads) void k_rs_hist_enc(int64_t n, int64_t seg, int shift, uint32_t *__restrict__ hist,
                                                            int nblocks, RsEncode enc) {
    constexpr int W = kRsThreads / 64;
    constexpr int NL = KES / 2;  // 16-B loads per 8-row group
    typedef long long v2 __attribute__((ext_vector_type(2)));
    __shared__ uint32_t h[W][kRadix];
    for (int i = threadIdx.x; i < W * kRadix; i += kRsThreads) (&h[0][0])[i] = 0;
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    const int64_t lo = (int64_t)blockIdx.x * seg, hi = lo + seg < n ? lo + seg : n;
    const bool asc = enc.asc != 0;
    const uint64_t emn = (uint64_t)enc.mn, emx = (uint64_t)enc.mx, bias = enc.bias, null_code = enc.null_code;
    uint32_t *hw = &h[wave][0];
    auto count = [=](int64_t x, bool ok) {
        const uint64_t code = ok ? (asc ? (uint64_t)x - emn + bias : emx - (uint64_t)x + bias) : null_code;
        atomicAdd(&hw[(uint32_t)(code >> shift) & (kRadix - 1)], 1u);
    };
    const int ns = enc.ns ? enc.ns : 1;
    for (int sg0 = 0; sg0 < ns; ++sg0) {
        // a scalar index into the kernel arguments (else the compiler copies RsEncode to scratch)
        const int sg = __builtin_amdgcn_readfirstlane(sg0);
        const ColRef c = enc.ns ? enc.sk[sg] : enc.c;
        const int64_t st = enc.ns ? enc.start[sg] : 0, en = enc.ns ? enc.start[sg + 1] : n;
        const int64_t a = (lo > st ? lo : st) - st, e = (hi < en ? hi : en) - st;  // local rows [a, e)
        if (a >= e) continue;
        auto row = [=](int64_t i) {
            const int64_t x = KES == 4 ? (int64_t)__builtin_nontemporal_load((const int32_t *)c.values + i)
                                       : __builtin_nontemporal_load((const int64_t *)c.values + i);
            count(x, col_valid(c, i));
        };
        const bool vec = ((uintptr_t)c.values & 15) == 0 && (!c.validity || (c.vbit0 & 7) == 0);
        int64_t ga = (a + 7) / 8, gb = e / 8;  // whole 8-row groups [ga, gb)
        if (!vec || ga >= gb) ga = gb = 0;
        const int64_t h0 = ga < gb ? ga * 8 : e, t0 = ga < gb ? gb * 8 : e;
        for (int64_t i = a + threadIdx.x; i < h0; i += kRsThreads) row(i);
        for (int64_t i = (t0 > a ? t0 : a) + threadIdx.x; i < e; i += kRsThreads) row(i);
        const uint8_t *vb = c.validity ? c.validity + (c.vbit0 >> 3) : nullptr;
        for (int64_t g0 = ga + threadIdx.x; g0 < gb; g0 += 4 * kRsThreads) {
            uint32_t m[4];
            v2 q[4][NL];
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                const bool live = g0 + w * kRsThreads < gb;
                const int64_t g = live ? g0 + w * kRsThreads : g0;
                m[w] = live ? (vb ? (uint32_t)vb[g] : 0xFFu) : 0u;
                const v2 *kv = (const v2 *)((const char *)c.values + g * 8 * KES);
#pragma unroll
                for (int u = 0; u < NL; ++u) q[w][u] = __builtin_nontemporal_load(kv + u);
            }
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                if (g0 + w * kRsThreads >= gb) continue;
#pragma unroll
                for (int r = 0; r < 8; ++r) {
                    int64_t x;
                    if constexpr (KES == 8) {
                        x = (r & 1) ? q[w][r >> 1].y : q[w][r >> 1].x;
                    } else {
                        const long long wd = (r & 2) ? q[w][r >> 2].y : q[w][r >> 2].x;
                        x = (int64_t)(int32_t)(uint32_t)((r & 1) ? ((unsigned long long)wd >> 32) : (unsigned long long)wd);
                    }
                    count(x, (m[w] >> r) & 1u);
                }
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < kRadix) {
        uint32_t cnt = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) cnt += h[w][threadIdx.x];
        hist[(int64_t)threadIdx.x * nblocks + blockIdx.x] = cnt;
    }
}

// Histogram of a pass whose digits the previous scatter wrote as a byte stream
// (nd_out): 1 B per element instead of the 8-B key, 16 digits per 16-B load,
// per-wave LDS counters (no cross-wave atomics on hot digits).
__global__ __launch_bounds__(kRsThreads) void k_rs_hist_u8(const uint8_t *__restrict__ dg, int64_t n, int64_t seg,
                                                           uint32_t *__restrict__ hist, int nblocks) {
    constexpr int W = kRsThreads / 64;
    __shared__ uint32_t h[W][kRadix];
    for (int i = threadIdx.x; i < W * kRadix; i += kRsThreads) (&h[0][0])[i] = 0;
    __syncthreads();
    const int wave = threadIdx.x >> 6;
    const int64_t lo = (int64_t)blockIdx.x * seg, hi = lo + seg < n ? lo + seg : n;
    // segments start at multiples of seg; the 16-B body is [a, b), head/tail bytewise
    const int64_t a = (lo + 15) & ~(int64_t)15, b = hi & ~(int64_t)15;
    if (a < b) {
        for (int64_t i = a + 16 * (int64_t)threadIdx.x; i < b; i += 16 * (int64_t)kRsThreads) {
            typedef unsigned int v4u32s __attribute__((ext_vector_type(4)));
            const v4u32s w = __builtin_nontemporal_load((const v4u32s *)(dg + i));
            const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int r = 0; r < 4; ++r) atomicAdd(&h[wave][(ws[q] >> (8 * r)) & 0xff], 1u);
        }
        for (int64_t i = lo + threadIdx.x; i < a; i += kRsThreads) atomicAdd(&h[wave][dg[i]], 1u);
        for (int64_t i = b + threadIdx.x; i < hi; i += kRsThreads) atomicAdd(&h[wave][dg[i]], 1u);
    } else {
        for (int64_t i = lo + threadIdx.x; i < hi; i += kRsThreads) atomicAdd(&h[wave][dg[i]], 1u);
    }
    __syncthreads();
    if (threadIdx.x < kRadix) {
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) c += h[w][threadIdx.x];
        hist[(int64_t)threadIdx.x * nblocks + blockIdx.x] = c;
    }
}

// Stable scatter, one 1024-thread workgroup per CU: rank each 8192-element
// tile by digit (ballot peers + per-wave counters), reorder it in LDS, then
// write every digit's run (≈ 32 elements = whole 128-byte lines) contiguously.
// Few, long-lived workgroups keep the open output lines of an XCD within its
// L2 (32 workgroups × 256 digits × 2 arrays), and the next tile's loads are
// issued before the current tile is ranked (LDS-only barriers below do not
// wait for them).

// The payload sort's last pass writes the decoded key column itself (DEC): code -> Int64 / Int32 value
// as rs_load_key's inverse, and one valid byte per row for the bitmap packed afterwards.
struct RsDecode {
    int64_t mn, mx;
    uint64_t bias, null_code;
    int32_t asc, dt;
    void *out;
    uint8_t *validb;  // nullable key: 1 = value, 0 = NULL (else nullptr)
};

// AT: tile ranks by LDS atomics (ds_add_rtn serves one instruction's lanes in lane order, so the
// rank is stable: tools/ubench/lds_order_ubench.hip), else by ballot peers (QEH_RS_BALLOT=1, A/B).
// ValT: the carried value -- a u32 row id, or (qeh_merge_sorted's payload sort) an 8-B payload.
// SEG (the MSD payload sort's second pass): block b's rows [lo, hi) and its offsets come from a
// segment table (lo, hi, hb, nbb per block): offsets[hb + digit * nbb], so every block stays inside
// one first-pass bucket and the scan orders (bucket, digit, block).
template <typename KeyT, bool AT = true, typename ValT = uint32_t, bool DEC = false, int KES = 0, bool SEG = false,
          typename KOutT = KeyT>
__global__ __launch_bounds__(kRsThreads) void k_rs_scatter(const KeyT *__restrict__ keys, const ValT *__restrict__ vals,
                                                           int64_t n, int64_t seg, int shift, const uint64_t *__restrict__ offs,
                                                           int nblocks, KOutT *__restrict__ keys_out,
                                                           ValT *__restrict__ vals_out, uint8_t *__restrict__ nd_out,
                                                           int nshift, RsDecode dec, RsEncode enc,
                                                           const int64_t *__restrict__ segtab = nullptr) {
    constexpr int W = kRsThreads / 64;
    constexpr int DW = kRadix / 64;       // waves that own one digit per lane in the bookkeeping
    __shared__ KeyT s_keys[kRsSTile];
    __shared__ ValT s_vals[kRsSTile];
    __shared__ uint32_t wcnt[W][kRadix];  // per-wave digit counts, then per-wave start inside the digit
    __shared__ uint32_t loc[kRadix];      // tile-local start of each digit
    __shared__ uint32_t tot_s[kRadix];
    __shared__ uint32_t wsum[DW];
    __shared__ uint64_t run[kRadix];      // global position of the block's next element of each digit
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    int64_t lo, hi;
    if constexpr (SEG) {
        const int64_t *e = segtab + 4 * (int64_t)blockIdx.x;
        lo = e[0], hi = e[1];
        if (t < kRadix) run[t] = offs[e[2] + (int64_t)t * e[3]];
    } else {
        if (t < kRadix) run[t] = offs[(int64_t)t * nblocks + blockIdx.x];
        lo = (int64_t)blockIdx.x * seg, hi = lo + seg < n ? lo + seg : n;
    }
    KeyT k[kRsIpt];
    ValT v[kRsIpt];
    // loads are unconditional (indices clamped into [lo, hi)): no branches around
    // them, so the compiler's wait counts stay exact and the prefetch really
    // stays in flight across the ranking of the current tile
    auto load_tile = [&](int64_t c0, KeyT *kk, ValT *vv) {
        const int64_t base = c0 + (int64_t)wave * 64 * kRsIpt + lane;
        const int ts = KES != 0 ? rs_tile_seg(enc, c0, (c0 + kRsSTile < hi ? c0 + kRsSTile : hi) - 1) : 0;
#pragma unroll
        for (int j = 0; j < kRsIpt; ++j) {
            const int64_t i = base + j * 64;
            const int64_t ii = i < hi ? i : hi - 1;
            kk[j] = rs_load_key<KES>(keys, enc, ii, ts);
            vv[j] = rs_load_val<KES>(vals, enc, ii, ts);
        }
    };
    if (lo < hi) load_tile(lo, k, v);
    for (int64_t c0 = lo; c0 < hi; c0 += kRsSTile) {
        for (int i = t; i < W * kRadix; i += kRsThreads) (&wcnt[0][0])[i] = 0;
        KeyT kn[kRsIpt];
        ValT vn[kRsIpt];
        const int64_t c1 = c0 + kRsSTile;
        load_tile(c1 < hi ? c1 : c0, kn, vn);  // in flight while this tile is ranked and written
        lds_barrier();
        const int64_t base = c0 + (int64_t)wave * 64 * kRsIpt + lane;
        uint32_t rk[kRsIpt];
#pragma unroll
        for (int j = 0; j < kRsIpt; ++j) {
            const bool live = base + j * 64 < hi;
            const uint32_t dg = (uint32_t)((k[j] >> shift) & (kRadix - 1));
            if constexpr (AT) {
                // LDS atomics serve the lanes of one instruction in lane order: the same stable rank
                rk[j] = live ? atomicAdd(&wcnt[wave][dg], 1u) : 0u;
            } else {
                const uint64_t peers = digit_peers(dg, live);
                const uint32_t before = wcnt[wave][dg];
                rk[j] = before + mbcnt(peers);
                if (live && mbcnt(peers) == 0) wcnt[wave][dg] = before + (uint32_t)popc64(peers);
            }
        }
        lds_barrier();
        // thread t < 256 = digit t: wave starts inside the digit, tile total, scan -> loc
        uint32_t tot = 0, incl = 0;
        if (t < kRadix) {
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const uint32_t c = wcnt[w][t];
                wcnt[w][t] = tot;
                tot += c;
            }
            tot_s[t] = tot;
            incl = wave_incl_scan(tot);
            if (lane == 63) wsum[wave] = incl;
        }
        lds_barrier();
        if (t < kRadix) {
            uint32_t wbase = 0;
#pragma unroll
            for (int w = 0; w < DW; ++w) wbase += w < wave ? wsum[w] : 0;
            loc[t] = wbase + incl - tot;
        }
        lds_barrier();
#pragma unroll
        for (int j = 0; j < kRsIpt; ++j) {
            if (base + j * 64 < hi) {
                const uint32_t dg = (uint32_t)((k[j] >> shift) & (kRadix - 1));
                const uint32_t p = loc[dg] + wcnt[wave][dg] + rk[j];
                s_keys[p] = k[j];
                s_vals[p] = v[j];
            }
        }
        lds_barrier();
        const int cnt = (int)(hi - c0 < kRsSTile ? hi - c0 : kRsSTile);
        for (int p = t; p < cnt; p += kRsThreads) {
            const KeyT key = s_keys[p];
            const uint32_t dg = (uint32_t)((key >> shift) & (kRadix - 1));
            const uint64_t pos = run[dg] + (uint64_t)(p - (int)loc[dg]);
            if constexpr (DEC) {
                const uint64_t c = (uint64_t)key;
                const bool ok = !dec.validb || c != dec.null_code;  // no NULLs: every code is a value
                const int64_t x = ok ? (dec.asc ? (int64_t)(c - dec.bias + (uint64_t)dec.mn)
                                               : (int64_t)((uint64_t)dec.mx - (c - dec.bias)))
                                     : 0;
                if (dec.dt == QEH_DT_INT32) ((int32_t *)dec.out)[pos] = (int32_t)x;
                else ((int64_t *)dec.out)[pos] = x;
                if (dec.validb) dec.validb[pos] = ok ? 1 : 0;
            } else {
                keys_out[pos] = (KOutT)key;  // (KOutT narrower: the low code bits the next stage needs)
            }
            vals_out[pos] = s_vals[p];
            if (nd_out) nd_out[pos] = (uint8_t)(key >> nshift);  // the next pass's digit (its histogram input)
        }
        lds_barrier();
        if (t < kRadix) run[t] += tot_s[t];
#pragma unroll
        for (int j = 0; j < kRsIpt; ++j) {
            k[j] = kn[j];
            v[j] = vn[j];
        }
    }
}

void launch_hist_u8(qeh_ctx *ctx, const uint8_t *ids, int64_t n, int64_t seg, uint32_t *hist, int nblocks) {
    hipLaunchKernelGGL(k_rs_hist_u8, dim3(nblocks), dim3(kRsThreads), 0, ctx->stream, ids, n, seg, hist, nblocks);
}

// The grid of the LSD passes over n rows and their histogram / offset buffers: one long-lived scatter
// workgroup per CU (see k_rs_scatter); hist uses the same segments.
struct RadixGrid {
    int nblocks = 0;
    int64_t seg = 0;
    DevBuf hist, offs;
    int init(qeh_ctx *ctx, int64_t n) {
        nblocks = (int)std::min<int64_t>(std::max<int64_t>((n + kRsSTile - 1) / kRsSTile, 1), (int64_t)ctx->props.multiProcessorCount);
        seg = (n + nblocks - 1) / nblocks;
        QEH_TRY(hist.alloc(ctx, (size_t)kRadix * nblocks * 4));
        return offs.alloc(ctx, (size_t)kRadix * nblocks * 8);
    }
};

// One stable pass on the 8-bit digit at `shift` (u32 / u64 keys as KeyT).  nd_in: the digits as the
// byte stream the previous scatter wrote (else read from the keys); nd_out: where this scatter
// writes the digits at `nshift` for the next pass (else nullptr).
template <typename KeyT>
static int radix_pass_t(qeh_ctx *ctx, RadixState &rs, RadixGrid &g, int shift, const uint8_t *nd_in, uint8_t *nd_out,
                        int nshift) {
    KernelTimer kt(ctx, "radix_pass");
    const int64_t n = rs.n;
    const int c = rs.cur;
    if (nd_in)
        launch_hist_u8(ctx, nd_in, n, g.seg, g.hist.as<uint32_t>(), g.nblocks);
    else
        hipLaunchKernelGGL(k_rs_hist<KeyT>, dim3(g.nblocks), dim3(kRsThreads), 0, ctx->stream, rs.k[c].as<KeyT>(), n, g.seg,
                           shift, g.hist.as<uint32_t>(), g.nblocks, RsEncode{});
    QEH_HIP(hipGetLastError());
    QEH_TRY(exclusive_scan_u32(ctx, g.hist.as<uint32_t>(), g.offs.as<uint64_t>(), (int64_t)kRadix * g.nblocks, nullptr));
    auto scat = rs_ballot(ctx) ? k_rs_scatter<KeyT, false> : k_rs_scatter<KeyT, true>;
    hipLaunchKernelGGL(scat, dim3(g.nblocks), dim3(kRsThreads), 0, ctx->stream, rs.k[c].as<KeyT>(), rs.v[c].as<uint32_t>(), n,
                       g.seg, shift, g.offs.as<uint64_t>(), g.nblocks, rs.k[1 - c].as<KeyT>(), rs.v[1 - c].as<uint32_t>(),
                       nd_out, nshift, RsDecode{}, RsEncode{}, nullptr);
    QEH_HIP(hipGetLastError());
    rs.cur = 1 - c;
    return QEH_OK;
}

static int radix_pass(qeh_ctx *ctx, RadixState &rs, RadixGrid &g, int shift, const uint8_t *nd_in, uint8_t *nd_out,
                      int nshift) {
    return rs.key32 ? radix_pass_t<uint32_t>(ctx, rs, g, shift, nd_in, nd_out, nshift)
                    : radix_pass_t<uint64_t>(ctx, rs, g, shift, nd_in, nd_out, nshift);
}

int radix_passes(qeh_ctx *ctx, RadixState &rs, int bits) {
    const int64_t n = rs.n;
    if (n <= 1 || bits <= 0) return QEH_OK;
    RadixGrid g;
    QEH_TRY(g.init(ctx, n));
    // every scatter but the last also writes the next pass's digit as one byte per element, so
    // that pass's histogram reads 1 B instead of the key (4 or 8 B)
    DevBuf nd;
    const bool multi = bits > kRadixBits && n >= (int64_t)kRsSTile;
    if (multi) QEH_TRY(nd.alloc(ctx, (size_t)n));
    for (int shift = 0; shift < bits; shift += kRadixBits) {
        const bool next = multi && shift + kRadixBits < bits;
        QEH_TRY(radix_pass(ctx, rs, g, shift, multi && shift > 0 ? nd.as<uint8_t>() : nullptr,
                           next ? nd.as<uint8_t>() : nullptr, shift + kRadixBits));
    }
    return QEH_OK;
}

int radix_pass_at(qeh_ctx *ctx, RadixState &rs, int shift) {
    if (rs.n <= 1) return QEH_OK;
    RadixGrid g;
    QEH_TRY(g.init(ctx, rs.n));
    return radix_pass(ctx, rs, g, shift, nullptr, nullptr, 0);
}

// Encode key column `c` through the current permutation (or identity) and
// sort by it.  Returns the key range bits used.
static int sort_by_column(qeh_ctx *ctx, RadixState &rs, const qeh_column &col, bool asc, bool first,
                          bool nulls_last = false) {
    const ColRef c = make_colref(col);
    const int64_t n = rs.n;  // == col.length (check_sort_keys)
    // min/max do not depend on row order: read the column directly, not through the permutation
    KeyStats ks{};
    QEH_TRY(sort_key_range(ctx, col, &ks.mn, &ks.mx));
    const bool nullable = col.validity != nullptr && col.null_count != 0;
    int bits = 1;  // all NULL (or empty)
    // NULLs first: NULL -> 0, values -> 1 .. span+1; NULLs last: values -> 0 .. span, NULL -> span+1
    uint64_t bias = (nullable && !nulls_last) ? 1 : 0;
    uint64_t null_code = 0;
    bool null_pass = false;
    if (ks.mn <= ks.mx) {
        const uint64_t span = (uint64_t)ks.mx - (uint64_t)ks.mn;
        if (nullable && span == UINT64_MAX) {  // 2^64 values + NULL: 65 bits -> separate null-flag pass
            bias = 0;
            null_pass = true;
        }
        const uint64_t top = span + ((nullable && !null_pass) ? 1 : 0);
        if (nullable && nulls_last && !null_pass) null_code = top;
        bits = bit_length(top);
        if (bits == 0) bits = 1;
    }
    for (int pass = 0; pass < (null_pass ? 2 : 1); ++pass) {
        const uint32_t *pm = (first && pass == 0) ? nullptr : rs.v[rs.cur].as<uint32_t>();
        const int o = 1 - rs.cur;  // encode into the spare buffers, then swap
        const int pbits = pass == 0 ? bits : 1;
        rs.key32 = pbits <= 32;  // narrow keys halve the key traffic of every pass
        {
            KernelTimer kt(ctx, "sort_encode");
            const int g = grid_for(ctx, n, kBlock * 8, 8);
            // the null-flag pass (pass 1) orders NULL vs value: code 1 for NULL when NULLs go last
            const uint64_t nc = pass == 0 ? null_code : (nulls_last ? 1 : 0);
            if (rs.key32)
                hipLaunchKernelGGL(k_encode<uint32_t>, dim3(g), dim3(kBlock), 0, ctx->stream, c, pm, n, ks.mn, ks.mx,
                                   asc ? 1 : 0, bias, pass, nc, rs.k[o].as<uint32_t>(), rs.v[o].as<uint32_t>());
            else
                hipLaunchKernelGGL(k_encode<uint64_t>, dim3(g), dim3(kBlock), 0, ctx->stream, c, pm, n, ks.mn, ks.mx,
                                   asc ? 1 : 0, bias, pass, nc, rs.k[o].as<uint64_t>(), rs.v[o].as<uint32_t>());
        }
        QEH_HIP(hipGetLastError());
        rs.cur = o;
        QEH_TRY(radix_passes(ctx, rs, pbits));
    }
    rs.enc_injective = !null_pass;
    return QEH_OK;
}

// ---- two-key sorts (ROW_NUMBER's PARTITION BY k ORDER BY v, ORDER BY a, b) ----------------
// One LSD sort over the pair encoding K = (enc(k) << bv) | (enc(v) >> shift)
// instead of one sort per column.  When the two ranges need more than 64 bits,
// v keeps only its top bv bits (total 48 or 64) and a fix-up pass sorts the
// runs of equal K (rare: rows that share k and the top bits of v) by the
// dropped low bits, ties by row index, so the order stays exact.
constexpr int64_t kPairMaxRun = 64;

__device__ __forceinline__ uint64_t enc_key(const ColRef &c, int64_t row, int64_t mn, int64_t mx, int asc) {
    const int64_t x = ordered_key(c, row);
    return asc ? (uint64_t)x - (uint64_t)mn : (uint64_t)mx - (uint64_t)x;
}

template <typename KeyT>
__global__ void k_encode_pair(ColRef a, ColRef b, int64_t n, int64_t amn, int64_t amx, int aasc, int64_t bmn, int64_t bmx,
                              int basc, int bv, int shift, KeyT *__restrict__ keys, uint32_t *__restrict__ perm) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t ka = enc_key(a, i, amn, amx, aasc), kb = enc_key(b, i, bmn, bmx, basc);
        keys[i] = (KeyT)((bv >= 64 ? 0ull : ka << bv) | (kb >> shift));
        perm[i] = (uint32_t)i;
    }
}

__global__ void k_fix_pair_runs(const uint64_t *__restrict__ K, uint32_t *__restrict__ perm, int64_t n, ColRef b, int64_t bmn,
                                int64_t bmx, int basc, int shift, uint32_t *overflow) {
    const uint64_t mask = (1ull << shift) - 1ull;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i + 1 < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t k = K[i];
        if (K[i + 1] != k || (i > 0 && K[i - 1] == k)) continue;  // not the start of a run of equal K
        int64_t j = i + 1;
        while (j + 1 < n && K[j + 1] == k && j - i < kPairMaxRun) ++j;
        if (j + 1 < n && K[j + 1] == k) {
            *overflow = 1u;  // a long run: the caller falls back to the per-column sort
            continue;
        }
        // stable LSD from the identity left the run in row order: insertion-sort it by the low bits
        for (int64_t a = i + 1; a <= j; ++a) {
            const uint32_t r = perm[a];
            const uint64_t lo = enc_key(b, r, bmn, bmx, basc) & mask;
            int64_t c = a - 1;
            while (c >= i) {
                const uint32_t rc = perm[c];
                const uint64_t lc = enc_key(b, rc, bmn, bmx, basc) & mask;
                if (lc < lo || (lc == lo && rc < r)) break;
                perm[c + 1] = rc;
                --c;
            }
            perm[c + 1] = r;
        }
    }
}

constexpr int kPairNotEligible = -1;

static int sort_perm_pair(qeh_ctx *ctx, const qeh_column &ca, const qeh_column &cb, bool aasc, bool basc, int64_t n,
                          RadixState &rs) {
    if (std::getenv("QEH_NO_PAIR_SORT")) return kPairNotEligible;
    if ((ca.validity && ca.null_count != 0) || (cb.validity && cb.null_count != 0)) return kPairNotEligible;
    const ColRef a = make_colref(ca), b = make_colref(cb);
    DevBuf st;
    QEH_TRY(st.alloc(ctx, 2 * sizeof(KeyStats) + 16));
    KeyStats ks[2];
    {
        KernelTimer kt(ctx, "sort_encode");
        KeyStats *d = st.as<KeyStats>();
        hipLaunchKernelGGL(k_stats_init, dim3(1), dim3(1), 0, ctx->stream, d);
        hipLaunchKernelGGL(k_stats_init, dim3(1), dim3(1), 0, ctx->stream, d + 1);
        const int g = grid_for(ctx, n, kBlock * 8, 1);
        hipLaunchKernelGGL(k_key_stats, dim3(g), dim3(kBlock), 0, ctx->stream, a, nullptr, n, d);
        hipLaunchKernelGGL(k_key_stats, dim3(g), dim3(kBlock), 0, ctx->stream, b, nullptr, n, d + 1);
    }
    QEH_HIP(hipGetLastError());
    QEH_TRY(read_small(ctx, ks, st.p, sizeof ks));
    const int ba = bit_length((uint64_t)ks[0].mx - (uint64_t)ks[0].mn);
    const int bb = bit_length((uint64_t)ks[1].mx - (uint64_t)ks[1].mn);
    int bv, shift, total;
    if (ba + bb <= 64) {
        bv = bb;
        shift = 0;
        total = ba + bb;
    } else if (ba <= 40) {
        // K keeps a's bits and the top bits of b; equal-K runs (fixed up exactly below) stay rare
        // when K has ~10 bits more than the row count needs: total = roundup8(log2 n + 10), at
        // least 16 bits of b, at most 64 (1e9 rows: 40 bits = 5 passes instead of 6)
        total = std::min(64, (bit_length((uint64_t)n) + 10 + 7) / 8 * 8);
        if (total < ba + 16) total = std::min(64, (ba + 16 + 7) / 8 * 8);
        if (total < 40) total = 40;  // 64-bit keys (k_fix_pair_runs reads them as such)
        bv = total - ba;
        shift = bb - bv;
    } else {
        return kPairNotEligible;
    }
    if (total == 0) total = 1;
    rs.key32 = total <= 32;
    {
        KernelTimer kt(ctx, "sort_encode");
        const int g = grid_for(ctx, n, kBlock * 8, 8);
        const int o = 1 - rs.cur;
        if (rs.key32)
            hipLaunchKernelGGL(k_encode_pair<uint32_t>, dim3(g), dim3(kBlock), 0, ctx->stream, a, b, n, ks[0].mn, ks[0].mx,
                               aasc ? 1 : 0, ks[1].mn, ks[1].mx, basc ? 1 : 0, bv, shift, rs.k[o].as<uint32_t>(),
                               rs.v[o].as<uint32_t>());
        else
            hipLaunchKernelGGL(k_encode_pair<uint64_t>, dim3(g), dim3(kBlock), 0, ctx->stream, a, b, n, ks[0].mn, ks[0].mx,
                               aasc ? 1 : 0, ks[1].mn, ks[1].mx, basc ? 1 : 0, bv, shift, rs.k[o].as<uint64_t>(),
                               rs.v[o].as<uint32_t>());
        rs.cur = o;
    }
    QEH_HIP(hipGetLastError());
    QEH_TRY(radix_passes(ctx, rs, total));
    if (shift > 0) {
        DevBuf flag;
        QEH_TRY(flag.alloc(ctx, 8));
        QEH_HIP(hipMemsetAsync(flag.p, 0, 8, ctx->stream));
        {
            KernelTimer kt(ctx, "sort_encode");
            hipLaunchKernelGGL(k_fix_pair_runs, dim3(grid_for(ctx, n, kBlock * 8, 8)), dim3(kBlock), 0, ctx->stream,
                               rs.k[rs.cur].as<uint64_t>(), rs.v[rs.cur].as<uint32_t>(), n, b, ks[1].mn, ks[1].mx,
                               basc ? 1 : 0, shift, flag.as<uint32_t>());
        }
        QEH_HIP(hipGetLastError());
        uint32_t of = 0;
        QEH_TRY(read_small(ctx, &of, flag.p, 4));
        if (of) return kPairNotEligible;
    }
    rs.enc_injective = false;
    rs.part_shift = bv;
    return QEH_OK;
}

// Stable lexicographic permutation by keys (last key sorted first).
int sort_perm(qeh_ctx *ctx, const qeh_column *keys, int n_keys, const int8_t *ascending, int64_t n, RadixState &rs,
              const int8_t *nulls_first) {
    rs.n = n;
    for (int b = 0; b < 2; ++b) {
        QEH_TRY(rs.k[b].alloc(ctx, (size_t)std::max<int64_t>(n, 1) * 8));
        QEH_TRY(rs.v[b].alloc(ctx, (size_t)std::max<int64_t>(n, 1) * 4));
    }
    rs.cur = 0;
    rs.part_shift = -1;
    if (n == 0) return QEH_OK;
    if (n_keys == 2) {
        const int r = sort_perm_pair(ctx, keys[0], keys[1], ascending ? ascending[0] != 0 : true,
                                     ascending ? ascending[1] != 0 : true, n, rs);
        if (r != kPairNotEligible) return r;
        rs.cur = 0;  // fall back: the per-column sort starts from the identity
        rs.part_shift = -1;
    }
    for (int j = n_keys - 1; j >= 0; --j)
        QEH_TRY(sort_by_column(ctx, rs, keys[j], ascending ? ascending[j] != 0 : true, j == n_keys - 1,
                               nulls_first ? nulls_first[j] == 0 : false));
    return QEH_OK;
}

int check_sort_keys(const qeh_column *keys, int n_keys, int64_t *n) {
    if (n_keys < 1) return fail(QEH_E_INVALID, "sort needs at least one key");
    *n = keys[0].length;
    for (int j = 0; j < n_keys; ++j) {
        QEH_TRY(check_column(keys[j], "sort key"));
        // Utf8 keys reach the sort as dictionary codes (encode_utf8_keys at the entry points)
        if (keys[j].dtype == QEH_DT_UTF8) return fail(QEH_E_INTERNAL, "Utf8 sort key was not dictionary-encoded");
        if (keys[j].length != *n) return fail(QEH_E_INVALID, "sort keys have different lengths");
    }
    return QEH_OK;
}

template <typename T>
__global__ void k_scatter(const T *__restrict__ src, const uint32_t *__restrict__ idx, int64_t m, T *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x)
        out[idx[i]] = src[i];
}

__global__ void k_u64_to_u32_idx(const int64_t *__restrict__ in, int64_t n, int64_t limit, uint32_t *__restrict__ out,
                                 uint32_t *__restrict__ bad) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t v = in[i];
        if (v < 0 || v >= limit) *bad = 1u;
        out[i] = (uint32_t)(v < 0 || v >= limit ? 0 : v);
    }
}

// ---- entry points for the top-k select (k_topk.hip) -------------------------------------------
__global__ void k_perm_prefix(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ rows, int64_t m,
                              uint32_t *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = rows ? rows[perm[i]] : perm[i];
}

int sort_key_range(qeh_ctx *ctx, const qeh_column &col, int64_t *mn, int64_t *mx) {
    DevBuf st;
    QEH_TRY(st.alloc(ctx, sizeof(KeyStats)));
    {
        KernelTimer kt(ctx, "sort_encode");
        hipLaunchKernelGGL(k_stats_init, dim3(1), dim3(1), 0, ctx->stream, st.as<KeyStats>());
        hipLaunchKernelGGL(k_key_stats, dim3(grid_for(ctx, col.length, kBlock * 8, 1)), dim3(kBlock), 0, ctx->stream,
                           make_colref(col), nullptr, col.length, st.as<KeyStats>());
    }
    QEH_HIP(hipGetLastError());
    KeyStats ks{};
    QEH_TRY(read_small(ctx, &ks, st.p, sizeof ks));
    *mn = ks.mn, *mx = ks.mx;
    return QEH_OK;
}

int sort_perm_prefix(qeh_ctx *ctx, const qeh_column *keys, int n_keys, const int8_t *ascending, int64_t n, int64_t limit,
                     const uint32_t *rows, qeh_column *out_perm) {
    RadixState rs;
    QEH_TRY(sort_perm(ctx, keys, n_keys, ascending, n, rs));
    const int64_t m = std::min(limit, n);
    QEH_TRY(alloc_column(ctx, QEH_DT_UINT32, m, false, out_perm));
    if (m > 0) {
        hipLaunchKernelGGL(k_perm_prefix, dim3(grid_for(ctx, m, kBlock * 8, 8)), dim3(kBlock), 0, ctx->stream,
                           rs.v[rs.cur].as<uint32_t>(), rows, m, (uint32_t *)out_perm->values);
        QEH_HIP(hipGetLastError());
    }
    QEH_HIP(hipStreamSynchronize(ctx->stream));  // rs's buffers return to the pool with this call
    return QEH_OK;
}

}  // namespace qeh

using namespace qeh;

// qeh_sort_indices / qeh_sort_indices_nulls (nulls_first == nullptr: NULLs first for every key)
static int sort_indices(qeh_ctx *ctx, const qeh_column *keys, int n_keys, const int8_t *ascending, const int8_t *nulls_first,
                        qeh_column *out_perm) {
    DeviceGuard dg(ctx->device);
    if (any_recoded_key(keys, n_keys)) {  // codes compare as the strings do; temporal keys as their integers
        Utf8Keys uk;
        QEH_TRY(encode_utf8_keys(ctx, keys, n_keys, &uk));
        return sort_indices(ctx, uk.keys.data(), n_keys, ascending, nulls_first, out_perm);
    }
    int64_t n;
    QEH_TRY(check_sort_keys(keys, n_keys, &n));
    RadixState rs;
    QEH_TRY(sort_perm(ctx, keys, n_keys, ascending, n, rs, nulls_first));
    QEH_TRY(alloc_column(ctx, QEH_DT_UINT32, n, false, out_perm));
    if (n > 0) QEH_HIP(hipMemcpyAsync(out_perm->values, rs.v[rs.cur].p, (size_t)n * 4, hipMemcpyDeviceToDevice, ctx->stream));
    QEH_HIP(hipStreamSynchronize(ctx->stream));
    return QEH_OK;
}

extern "C" int qeh_sort_indices(qeh_ctx *ctx, const qeh_column *keys, int n_keys, const int8_t *ascending,
                                qeh_column *out_perm) {
    if (!ctx || !keys || !out_perm) return fail(QEH_E_INVALID, "qeh_sort_indices: bad argument");
    return sort_indices(ctx, keys, n_keys, ascending, nullptr, out_perm);
}

extern "C" int qeh_sort_indices_nulls(qeh_ctx *ctx, const qeh_column *keys, int n_keys, const int8_t *ascending,
                                      const int8_t *nulls_first, qeh_column *out_perm) {
    if (!ctx || !keys || !out_perm) return fail(QEH_E_INVALID, "qeh_sort_indices_nulls: bad argument");
    return sort_indices(ctx, keys, n_keys, ascending, nulls_first, out_perm);
}

// ---- payload-carrying sort (qeh_merge_sorted of one Int64 / Int32 key and one 8-byte column) ----
// The key is encoded as in sort_by_column (asc: x - mn, desc: mx - x; NULL = 0 below every value
// code when NULLs go first, or above them when last) and sorted with the payload itself as the carried
// value, so no permutation is gathered afterwards: the sorted key column is decoded from the sorted
// codes, and the last pass writes the payload straight into the output column.

// valid bytes (the last pass's, one per row, each 0 or 1) -> the key's validity bitmap: one 64-row word
// per thread from four 16-B loads (bit i of a dword's 4 flags = bit 8 i of the dword)
__global__ void k_pack_valid(const uint8_t *__restrict__ vb, int64_t n, uint64_t *__restrict__ valid) {
    typedef unsigned int v4u32p __attribute__((ext_vector_type(4)));
    const int64_t nw = (n + 63) >> 6;
    for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < nw; w += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r0 = w << 6;
        uint64_t m = 0;
        if (r0 + 64 <= n) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const v4u32p x = __builtin_nontemporal_load((const v4u32p *)(vb + r0) + q);
                const uint32_t d[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    const uint32_t y = d[t];
                    const uint32_t b4 = (y & 1u) | ((y >> 7) & 2u) | ((y >> 14) & 4u) | ((y >> 21) & 8u);
                    m |= (uint64_t)b4 << (q * 16 + t * 4);
                }
            }
        } else {
            for (int64_t i = r0; i < n; ++i) m |= (uint64_t)(vb[i] != 0) << (i - r0);
        }
        valid[w] = m;
    }
}

// ---- MSD payload sort ----------------------------------------------------------------------
// Codes of 24..45 bits over >= 2^20 rows: two stable 256-way passes on the top 16 bits (k_rs_scatter
// over the whole array, then the same scatter inside every first-pass bucket: SEG blocks never straddle
// a bucket and the scan orders (bucket, digit, block)), then one workgroup per sub-bucket sorts its
// rows by the remaining low bits in LDS -- stable 8-bit LDS passes over (low code, row) pairs, ranks
// by lane-ordered LDS atomics as the global passes -- and writes the decoded key, the payload
// (gathered inside the sub-bucket) and the valid byte.  Three passes over the rows instead of
// ceil(bits / 8) hist + scatter pairs.  A sub-bucket above kMsdCap rows is copied through when its
// codes are all equal (the NULLs, a repeated key), else the caller redoes the sort on the LSD path.
constexpr int kMsdCap = 4096;
constexpr int kMsdThreads = 512;
constexpr int kMsdBits = 16;  // code bits the two global passes consume
constexpr uint32_t kMsdMaxBig = 255;  // sub-buckets above kMsdCap rows handled by k_msd_big
constexpr int kMsdLdsBits = 9;        // digit of the in-LDS passes: 25 low bits in three passes
constexpr int kMsdMaxLow = 29;        // low code bits the LDS sort packs beside a 12-bit row index

__global__ __launch_bounds__(kRsThreads) void k_rs_hist_u8_seg(const uint8_t *__restrict__ dg, const int64_t *__restrict__ segtab,
                                                               uint32_t *__restrict__ hist) {
    constexpr int W = kRsThreads / 64;
    __shared__ uint32_t h[W][kRadix];
    for (int i = threadIdx.x; i < W * kRadix; i += kRsThreads) (&h[0][0])[i] = 0;
    __syncthreads();
    const int64_t *e = segtab + 4 * (int64_t)blockIdx.x;
    const int64_t lo = e[0], hi = e[1];
    const int wave = threadIdx.x >> 6;
    const int64_t a = std::min<int64_t>(hi, (lo + 15) & ~(int64_t)15), b = std::max<int64_t>(a, hi & ~(int64_t)15);
    for (int64_t i = lo + threadIdx.x; i < a; i += kRsThreads) atomicAdd(&h[wave][dg[i]], 1u);
    for (int64_t i = b + threadIdx.x; i < hi; i += kRsThreads) atomicAdd(&h[wave][dg[i]], 1u);
    for (int64_t i = a + 16 * (int64_t)threadIdx.x; i < b; i += 16 * (int64_t)kRsThreads) {
        typedef unsigned int v4u32s __attribute__((ext_vector_type(4)));
        const v4u32s w = __builtin_nontemporal_load((const v4u32s *)(dg + i));
        const uint32_t ws[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int r = 0; r < 4; ++r) atomicAdd(&h[wave][(ws[q] >> (8 * r)) & 0xff], 1u);
    }
    __syncthreads();
    if (threadIdx.x < kRadix) {
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) c += h[w][threadIdx.x];
        hist[e[2] + (int64_t)threadIdx.x * e[3]] = c;
    }
}

// sub-bucket (bucket b, digit d) starts: the scanned second-pass offset of the bucket's first block
// (btab per bucket: hist base, blocks, start); sb[65536] = n
__global__ void k_msd_sbstart(const uint64_t *__restrict__ offs2, const int64_t *__restrict__ btab, int64_t n,
                              uint64_t *__restrict__ sb) {
    const int id = blockIdx.x * blockDim.x + threadIdx.x;
    if (id > kRadix * kRadix) return;
    if (id == kRadix * kRadix) {
        sb[id] = (uint64_t)n;
        return;
    }
    const int b = id >> kRadixBits, d = id & (kRadix - 1);
    const int64_t base = btab[3 * b], nb = btab[3 * b + 1];
    sb[id] = nb ? offs2[base * kRadix + (int64_t)d * nb] : (uint64_t)btab[3 * b + 2];
}

__device__ __forceinline__ void msd_emit(const RsDecode &dec, uint64_t *__restrict__ vout, int64_t pos, uint64_t c,
                                         uint64_t val) {
    const bool ok = !dec.validb || c != dec.null_code;
    const int64_t x = ok ? (dec.asc ? (int64_t)(c - dec.bias + (uint64_t)dec.mn) : (int64_t)((uint64_t)dec.mx - (c - dec.bias)))
                         : 0;
    if (dec.dt == QEH_DT_INT32) ((int32_t *)dec.out)[pos] = (int32_t)x;
    else ((int64_t *)dec.out)[pos] = x;
    if (dec.validb) dec.validb[pos] = ok ? 1 : 0;
    vout[pos] = val;
}

// one workgroup per sub-bucket (blockIdx.x = bucket << 8 | digit): the codes here share their top 16
// bits; pass 2 left their low 32 bits.  Rows e = wave * 64 J + j * 64 + lane keep input order in
// (wave, j, lane).  The first LDS pass ranks (low code, row e) and leaves packed words
// (remaining code bits << 12 | e), so the later passes move one dword per row (lbits <= 29).
// list (optional): only the sub-buckets list[1 .. list[0]] (the ones k_msd_csort queued), one per
// workgroup; else sub-bucket blockIdx.x
__global__ __launch_bounds__(kMsdThreads) void k_msd_lds_sort(const uint32_t *__restrict__ codes, const uint64_t *__restrict__ vin,
                                                              const uint64_t *__restrict__ sb, int lbits, RsDecode dec,
                                                              uint64_t *__restrict__ vout, uint32_t *__restrict__ flag,
                                                              uint32_t *__restrict__ big, const uint32_t *__restrict__ list) {
    constexpr int W = kMsdThreads / 64, J = kMsdCap / kMsdThreads;
    constexpr int DB = kMsdLdsBits, ND = 1 << DB, DPT = ND / kMsdThreads;  // digits per thread in the scan
    static_assert(DPT >= 1, "one digit per thread at least");
    constexpr int IB = 12;                                                 // row bits (kMsdCap = 2^12)
    static_assert(kMsdCap == 1 << IB, "row index bits");
    __shared__ uint32_t buf[2][kMsdCap];
    __shared__ uint32_t wc[W][ND];
    __shared__ uint32_t loc[ND], wsum[W];
    const uint32_t nlist = list ? list[0] : 0u;
    // list mode: the grid strides over the queued sub-buckets; else sub-bucket blockIdx.x
    for (uint32_t it = blockIdx.x; list ? it < nlist : it == blockIdx.x; it += gridDim.x) {
    const uint32_t id = list ? list[1 + it] : it;
    const int64_t s0 = (int64_t)sb[id], s1 = (int64_t)sb[id + 1];
    const int64_t m = s1 - s0;
    if (m <= 0) continue;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    if (m > kMsdCap) {  // k_msd_big takes it, with the whole grid
        if (t == 0) {
            const uint32_t q = atomicAdd(big, 1u);
            if (q < kMsdMaxBig) big[1 + q] = id;
            else atomicOr(flag, 1u);
        }
        continue;
    }
    const int mm = (int)m;
    const uint64_t hi_code = (uint64_t)id << lbits;
    const uint32_t lmask = lbits >= 32 ? 0xFFFFFFFFu : ((1u << lbits) - 1u);
    for (int e = t; e < mm; e += kMsdThreads) buf[0][e] = codes[s0 + e] & lmask;
    int cur = 0;
    for (int sh = 0; sh < lbits; sh += DB) {
        const bool first = sh == 0;
        for (int i = t; i < W * ND; i += kMsdThreads) (&wc[0][0])[i] = 0;
        __syncthreads();
        uint32_t kk[J], rk[J];
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int e = wave * 64 * J + j * 64 + lane;
            const bool live = e < mm;
            kk[j] = live ? buf[cur][e] : 0u;
            // the first pass reads raw low codes; later passes packed words (digit above the row bits)
            const uint32_t dg = first ? (kk[j] & (ND - 1)) : ((kk[j] >> IB) & (ND - 1));
            rk[j] = live ? atomicAdd(&wc[wave][dg], 1u) : 0u;
        }
        __syncthreads();
        // thread t owns digits t * DPT .. + DPT - 1: wave starts inside each digit, then one scan
        uint32_t dt[DPT], tot = 0;
#pragma unroll
        for (int q = 0; q < DPT; ++q) {
            const int d = t * DPT + q;
            uint32_t c0 = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const uint32_t c = wc[w][d];
                wc[w][d] = c0;
                c0 += c;
            }
            dt[q] = c0;
            tot += c0;
        }
        const uint32_t inc = wave_incl_scan(tot);
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        uint32_t wb = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) wb += w < wave ? wsum[w] : 0u;
        uint32_t run = wb + inc - tot;
#pragma unroll
        for (int q = 0; q < DPT; ++q) {
            loc[t * DPT + q] = run;
            run += dt[q];
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < J; ++j) {
            const int e = wave * 64 * J + j * 64 + lane;
            if (e >= mm) continue;
            const uint32_t dg = first ? (kk[j] & (ND - 1)) : ((kk[j] >> IB) & (ND - 1));
            const uint32_t p = loc[dg] + wc[wave][dg] + rk[j];
            // packed: the code bits above this pass's digit, then the row
            buf[cur ^ 1][p] = first ? (((kk[j] >> DB) << IB) | (uint32_t)e)
                                    : ((((kk[j] >> IB) >> DB) << IB) | (kk[j] & (kMsdCap - 1)));
        }
        __syncthreads();
        cur ^= 1;
    }
    // every pass ran (lbits > 0): buf holds rows in code order; the code is re-read from the row
    for (int e = t; e < mm; e += kMsdThreads) {
        const uint32_t r = buf[cur][e] & (kMsdCap - 1);
        msd_emit(dec, vout, s0 + e, hi_code | (codes[s0 + r] & lmask), vin[s0 + r]);
    }
    __syncthreads();  // (list mode: buf is read before the next sub-bucket overwrites it)
    }
}

// Counting sort of a sub-bucket in one LDS pass (replaces the three radix passes of k_msd_lds_sort for
// spread codes): 2^12 buckets of the top bits of the remaining code, each row placed by its bucket's
// start + arrival beside its (code, row) word, then ranked exactly among its bucket's rows by
// (code, row) -- the row order within equal codes is the input order, as the radix passes keep it.
// The ranked words then move to their sorted slots in LDS, and the output is written in sorted order
// (coalesced stores, the payload gathered by row): scattered stores measured 5.20 ms for the
// Merge::sorted shape against 4.09 ms for the radix passes, sorted-order stores 3.93 ms.
// A sub-bucket with a bucket above kCsCap rows (clustered or repeated codes) is queued in fb for
// k_msd_lds_sort (list mode); one above kMsdCap rows goes to k_msd_big as before.
// 12 bits measured best: 10 / 11 / 13 / 14 bits 3.96 / 3.85 / 4.05 / 5.06 ms vs 3.76, and 13 bits again
// with 32-bit rank words 3.71 vs 3.62 (ab_merge_csort.txt)
constexpr int kCsBits = 12, kCsCap = 24;
static_assert(kMsdCap <= 4096 && (kMsdCap & (kMsdCap - 1)) == 0, "row index packs into the low 12 bits");
template <int CB>
__global__ __launch_bounds__(kMsdThreads) void k_msd_csort(const uint32_t *__restrict__ codes, const uint64_t *__restrict__ vin,
                                                           const uint64_t *__restrict__ sb, int lbits, RsDecode dec,
                                                           uint64_t *__restrict__ vout, uint32_t *__restrict__ flag,
                                                           uint32_t *__restrict__ big, uint32_t *__restrict__ fb) {
    constexpr int W = kMsdThreads / 64, J = kMsdCap / kMsdThreads, NB = 1 << CB, BPT = NB / kMsdThreads;
    static_assert(NB >= kMsdCap, "cnt holds the sorted codes at the end");
    __shared__ uint32_t cnt[NB];      // counts, then starts; at the end the codes in sorted order
    __shared__ uint32_t ce[kMsdCap];  // by slot: the code bits below the bucket's << 12 | row; then rows in sorted order
    __shared__ uint32_t wsum[W], wmax[W];
    const int64_t s0 = (int64_t)sb[blockIdx.x], s1 = (int64_t)sb[blockIdx.x + 1];
    const int64_t m = s1 - s0;
    if (m <= 0) return;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    if (m > kMsdCap) {
        if (t == 0) {
            const uint32_t q = atomicAdd(big, 1u);
            if (q < kMsdMaxBig) big[1 + q] = blockIdx.x;
            else atomicOr(flag, 1u);
        }
        return;
    }
    const int mm = (int)m;
    const uint64_t hi_code = (uint64_t)blockIdx.x << lbits;
    const uint32_t lmask = lbits >= 32 ? 0xFFFFFFFFu : ((1u << lbits) - 1u);
    const int bshift = lbits > CB ? lbits - CB : 0;
    const uint32_t lowm = (1u << bshift) - 1u;  // bshift <= kMsdMaxLow - CB: the rank words fit 32 bits
    static_assert(kMsdMaxLow - CB + 12 <= 32, "rank words: low code bits + 12-bit row");
    for (int i = t; i < NB; i += kMsdThreads) cnt[i] = 0;
    uint32_t c[J], arr[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int e = j * kMsdThreads + t;
        c[j] = e < mm ? codes[s0 + e] & lmask : 0u;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int e = j * kMsdThreads + t;
        arr[j] = e < mm ? atomicAdd(&cnt[c[j] >> bshift], 1u) : 0u;
    }
    __syncthreads();
    {  // exclusive scan of the NB counts: thread t owns t * BPT .. + BPT - 1; the largest count on the side
        uint32_t w[BPT], tot = 0, mx = 0;
#pragma unroll
        for (int q = 0; q < BPT; ++q) {
            w[q] = cnt[t * BPT + q];
            tot += w[q];
            mx = max(mx, w[q]);
        }
        const uint32_t inc = wave_incl_scan(tot);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, d, 64));
        if (lane == 63) wsum[wave] = inc;
        if (lane == 0) wmax[wave] = mx;
        __syncthreads();
        uint32_t run = inc - tot;
        for (int v = 0; v < wave; ++v) run += wsum[v];
#pragma unroll
        for (int q = 0; q < BPT; ++q) {
            cnt[t * BPT + q] = run;
            run += w[q];
        }
    }
    uint32_t mxall = 0;
#pragma unroll
    for (int v = 0; v < W; ++v) mxall = max(mxall, wmax[v]);
    if (mxall > (uint32_t)kCsCap) {  // (uniform) clustered codes: the radix passes sort this one
        if (t == 0) fb[1 + atomicAdd(&fb[0], 1u)] = blockIdx.x;
        return;
    }
    __syncthreads();
    uint32_t slot[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int e = j * kMsdThreads + t;
        slot[j] = 0;
        if (e < mm) {
            slot[j] = cnt[c[j] >> bshift] + arr[j];
            ce[slot[j]] = ((c[j] & lowm) << 12) | (uint32_t)e;
        }
    }
    __syncthreads();
    uint32_t rank[J];
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int e = j * kMsdThreads + t;
        rank[j] = 0;
        if (e >= mm) continue;
        const uint32_t b = c[j] >> bshift;
        const uint32_t st = cnt[b], en = b + 1 < (uint32_t)NB ? cnt[b + 1] : (uint32_t)mm;
        const uint32_t me = ((c[j] & lowm) << 12) | (uint32_t)e;  // (a bucket shares the bits above)
        uint32_t rk = st;
        for (uint32_t x = st; x < en; ++x) rk += ce[x] < me ? 1u : 0u;
        rank[j] = rk;
    }
    __syncthreads();  // every rank read its bucket: the entries move to their sorted places
#pragma unroll
    for (int j = 0; j < J; ++j) {
        const int e = j * kMsdThreads + t;
        if (e < mm) {
            ce[rank[j]] = (uint32_t)e;
            cnt[rank[j]] = c[j];
        }
    }
    __syncthreads();
    // written in sorted order (coalesced), the payload gathered from its row
    for (int p = t; p < mm; p += kMsdThreads) msd_emit(dec, vout, s0 + p, hi_code | cnt[p], vin[s0 + ce[p]]);
}

// The sub-buckets above kMsdCap rows (big[0] of them, ids in big[1..]), every workgroup of the grid on
// each in turn: rows whose codes all equal the first one (the NULLs, one repeated key) are already in
// order and are copied through; any other code sets the redo flag (the LSD passes then rewrite all).
__global__ __launch_bounds__(256) void k_msd_big(const uint32_t *__restrict__ codes, const uint64_t *__restrict__ vin,
                                                 const uint64_t *__restrict__ sb, int lbits, RsDecode dec, uint64_t *__restrict__ vout,
                                                 uint32_t *__restrict__ flag, const uint32_t *__restrict__ big) {
    const uint32_t nbig = big[0] < kMsdMaxBig ? big[0] : kMsdMaxBig;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (uint32_t q = 0; q < nbig; ++q) {
        const uint32_t id = big[1 + q];
        const int64_t s0 = (int64_t)sb[id], s1 = (int64_t)sb[id + 1];
        const uint32_t c0 = codes[s0];
        const uint64_t full = ((uint64_t)id << lbits) | c0;
        bool bad = false;
        for (int64_t i = s0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < s1; i += stride) {
            if (codes[i] != c0) bad = true;
            else msd_emit(dec, vout, i, full, vin[i]);
        }
        if (bad) atomicOr(flag, 1u);
    }
}

// Returns QEH_OK (outputs written, validity bytes in validb) or kMsdRedo (a sub-bucket too large to
// sort in LDS: the caller runs the LSD passes over the same buffers).
constexpr int kMsdRedo = -5;
static int msd_payload_passes(qeh_ctx *ctx, const qeh_column &key, const uint64_t *vsrc, int64_t n, int bits, const RsEncode &enc,
                              const RsDecode &dec, uint64_t *kb0, uint64_t *kb1, uint64_t *vtmp, uint64_t *vout) {
    const bool k32 = key.dtype == QEH_DT_INT32;
    const int cus = ctx->props.multiProcessorCount;
    const int nblocks = (int)std::min<int64_t>(std::max<int64_t>((n + kRsSTile - 1) / kRsSTile, 1), (int64_t)cus);
    const int64_t seg = (n + nblocks - 1) / nblocks;
    const int shift1 = bits - kRadixBits, shift2 = bits - kMsdBits;
    DevBuf hist, offs, nd, vtmp2, tabd, btabd, sbd, flag, fbl;
    QEH_TRY(hist.alloc(ctx, (size_t)kRadix * nblocks * 4));
    QEH_TRY(offs.alloc(ctx, (size_t)kRadix * nblocks * 8));
    QEH_TRY(nd.alloc(ctx, (size_t)n + 16));
    QEH_TRY(vtmp2.alloc(ctx, (size_t)n * 8));
    QEH_TRY(sbd.alloc(ctx, ((size_t)kRadix * kRadix + 1) * 8));
    QEH_TRY(flag.alloc(ctx, 8 + 4 * (kMsdMaxBig + 1)));
    QEH_TRY(fbl.alloc(ctx, 4 * ((size_t)kRadix * kRadix + 1)));
    {
        KernelTimer kt(ctx, "radix_pass");
        if (std::getenv("QEH_RS_HIST_LANE")) {  // (A/B: the lane-strided histogram of the scatter's layout)
            auto hk = k32 ? k_rs_hist<uint64_t, 4> : k_rs_hist<uint64_t, 8>;
            hipLaunchKernelGGL(hk, dim3(nblocks), dim3(kRsThreads), 0, ctx->stream, kb0, n, seg, shift1, hist.as<uint32_t>(), nblocks,
                               enc);
        } else {
            auto hk = k32 ? k_rs_hist_enc<4> : k_rs_hist_enc<8>;
            hipLaunchKernelGGL(hk, dim3(nblocks), dim3(kRsThreads), 0, ctx->stream, n, seg, shift1, hist.as<uint32_t>(), nblocks, enc);
        }
        QEH_TRY(exclusive_scan_u32(ctx, hist.as<uint32_t>(), offs.as<uint64_t>(), (int64_t)kRadix * nblocks, nullptr));
        // the codes leave as their low 32 bits (the second pass takes its digit from the byte stream nd)
        auto sk = k32 ? k_rs_scatter<uint64_t, true, uint64_t, false, 4, false, uint32_t>
                      : k_rs_scatter<uint64_t, true, uint64_t, false, 8, false, uint32_t>;
        hipLaunchKernelGGL(sk, dim3(nblocks), dim3(kRsThreads), 0, ctx->stream, kb0, vsrc, n, seg, shift1, offs.as<uint64_t>(),
                           nblocks, (uint32_t *)kb1, vtmp, nd.as<uint8_t>(), shift2, dec, enc, nullptr);
        QEH_HIP(hipGetLastError());
    }
    // the buckets' starts (the scanned offsets of block 0), then blocks of <= S rows inside each bucket
    std::vector<uint64_t> bst(kRadix + 1);
    QEH_HIP(hipMemcpy2DAsync(bst.data(), 8, offs.p, (size_t)nblocks * 8, 8, kRadix, hipMemcpyDeviceToHost, ctx->stream));
    QEH_HIP(hipStreamSynchronize(ctx->stream));
    bst[kRadix] = (uint64_t)n;
    // ~4 blocks per CU: the buckets differ in size, so many shorter blocks balance the last round
    const int64_t S = std::max<int64_t>(kRsSTile, ((n + 4 * cus - 1) / (4 * cus) + kRsSTile - 1) / kRsSTile * kRsSTile);
    std::vector<int64_t> tab, btab;
    int64_t base = 0;
    for (int b = 0; b < kRadix; ++b) {
        const int64_t lo = (int64_t)bst[b], hi = (int64_t)bst[b + 1], size = hi - lo;
        const int64_t nb = size > 0 ? (size + S - 1) / S : 0;
        for (int64_t j = 0; j < nb; ++j) {
            tab.push_back(lo + j * S);
            tab.push_back(std::min<int64_t>(lo + (j + 1) * S, hi));
            tab.push_back(base * kRadix + j);
            tab.push_back(nb);
        }
        btab.push_back(base);
        btab.push_back(nb);
        btab.push_back(lo);
        base += nb;
    }
    const int64_t B = base;
    QEH_TRY(tabd.alloc(ctx, tab.size() * 8));
    QEH_TRY(btabd.alloc(ctx, btab.size() * 8));
    QEH_HIP(hipMemcpyAsync(tabd.p, tab.data(), tab.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    QEH_HIP(hipMemcpyAsync(btabd.p, btab.data(), btab.size() * 8, hipMemcpyHostToDevice, ctx->stream));
    DevBuf hist2, offs2;
    QEH_TRY(hist2.alloc(ctx, (size_t)kRadix * B * 4));
    QEH_TRY(offs2.alloc(ctx, (size_t)kRadix * B * 8));
    {
        KernelTimer kt(ctx, "radix_pass");
        hipLaunchKernelGGL(k_rs_hist_u8_seg, dim3((unsigned)B), dim3(kRsThreads), 0, ctx->stream, nd.as<uint8_t>(), tabd.as<int64_t>(),
                           hist2.as<uint32_t>());
        QEH_TRY(exclusive_scan_u32(ctx, hist2.as<uint32_t>(), offs2.as<uint64_t>(), (int64_t)kRadix * B, nullptr));
        uint32_t *codes2 = (uint32_t *)kb0;  // the low 32 code bits: all the LDS sort needs (lbits <= 29)
        RsEncode enc2{};  // codes = (nd << shift2) | low shift2 bits of the first pass's 32-bit codes
        enc2.nd = nd.as<uint8_t>();
        enc2.nd_shift = shift2;
        hipLaunchKernelGGL((k_rs_scatter<uint64_t, true, uint64_t, false, 1, true, uint32_t>), dim3((unsigned)B), dim3(kRsThreads), 0,
                           ctx->stream, kb1, vtmp, n, 0, shift2, offs2.as<uint64_t>(), (int)B, codes2, vtmp2.as<uint64_t>(), nullptr, 0,
                           dec, enc2, tabd.as<int64_t>());
        hipLaunchKernelGGL(k_msd_sbstart, dim3((kRadix * kRadix + 256) / 256), dim3(256), 0, ctx->stream, offs2.as<uint64_t>(),
                           btabd.as<int64_t>(), n, sbd.as<uint64_t>());
        QEH_HIP(hipMemsetAsync(flag.p, 0, 16, ctx->stream));
        uint32_t *bigl = flag.as<uint32_t>() + 2;
        if (std::getenv("QEH_MSD_RADIX_LDS")) {  // (A/B: the three-pass radix sort for every sub-bucket)
            hipLaunchKernelGGL(k_msd_lds_sort, dim3(kRadix * kRadix), dim3(kMsdThreads), 0, ctx->stream, codes2,
                               vtmp2.as<uint64_t>(), sbd.as<uint64_t>(), shift2, dec, vout, flag.as<uint32_t>(), bigl,
                               (const uint32_t *)nullptr);
        } else {
            // one counting pass per sub-bucket; the ones with a crowded bucket queued for the radix passes
            QEH_HIP(hipMemsetAsync(fbl.p, 0, 4, ctx->stream));
            hipLaunchKernelGGL(k_msd_csort<kCsBits>, dim3(kRadix * kRadix), dim3(kMsdThreads), 0, ctx->stream, codes2, vtmp2.as<uint64_t>(),
                               sbd.as<uint64_t>(), shift2, dec, vout, flag.as<uint32_t>(), bigl, fbl.as<uint32_t>());
            hipLaunchKernelGGL(k_msd_lds_sort, dim3(cus * 4), dim3(kMsdThreads), 0, ctx->stream, codes2,
                               vtmp2.as<uint64_t>(), sbd.as<uint64_t>(), shift2, dec, vout, flag.as<uint32_t>(), bigl,
                               (const uint32_t *)fbl.as<uint32_t>());
        }
        hipLaunchKernelGGL(k_msd_big, dim3(cus * 4), dim3(256), 0, ctx->stream, codes2, vtmp2.as<uint64_t>(), sbd.as<uint64_t>(),
                           shift2, dec, vout, flag.as<uint32_t>(), bigl);
        QEH_HIP(hipGetLastError());
    }
    uint32_t redo = 0;
    QEH_TRY(read_small(ctx, &redo, flag.p, 4));
    return redo ? kMsdRedo : QEH_OK;
}

int qeh::sort_pairs_payload(qeh_ctx *ctx, const qeh_column &key, const qeh_column &val, bool asc, bool nulls_first,
                            qeh_column *out_key, qeh_column *out_val) {
    return sort_pairs_payload_parts(ctx, &key, &val, 1, asc, nulls_first, out_key, out_val);
}

// The key / payload as nparts row segments (Merge::sorted's partitions, concatenated in order): the first
// pass reads them in place (RsEncode.ns); every later pass works on the sort's own buffers.
int qeh::sort_pairs_payload_parts(qeh_ctx *ctx, const qeh_column *keys, const qeh_column *vals, int nparts, bool asc,
                                  bool nulls_first, qeh_column *out_key, qeh_column *out_val) {
    if (nparts < 1 || nparts > kRsMaxSegs) return kPayloadSortNotEligible;
    const qeh_column &key = keys[0], &val = vals[0];
    int64_t n = 0;
    bool nullable = false;
    for (int p = 0; p < nparts; ++p) {
        if (keys[p].dtype != key.dtype || vals[p].dtype != val.dtype || vals[p].length != keys[p].length)
            return kPayloadSortNotEligible;
        if (vals[p].validity && vals[p].null_count != 0) return kPayloadSortNotEligible;
        nullable = nullable || (keys[p].validity && keys[p].null_count != 0);
        n += keys[p].length;
    }
    if (std::getenv("QEH_NO_PAYLOAD_SORT") || n <= 1 || n >= ((int64_t)1 << 32)) return kPayloadSortNotEligible;
    if (key.dtype != QEH_DT_INT64 && key.dtype != QEH_DT_INT32) return kPayloadSortNotEligible;
    if (rs_ballot(ctx)) return kPayloadSortNotEligible;  // its passes rank by LDS atomics only
    if (val.dtype != QEH_DT_INT64 && val.dtype != QEH_DT_FLOAT64) return kPayloadSortNotEligible;
    const ColRef kc = make_colref(key);
    DevBuf st;
    QEH_TRY(st.alloc(ctx, sizeof(KeyStats)));
    KeyStats ks{};
    {
        KernelTimer kt(ctx, "sort_encode");
        hipLaunchKernelGGL(k_stats_init, dim3(1), dim3(1), 0, ctx->stream, st.as<KeyStats>());
        if (nparts == 1) {
            hipLaunchKernelGGL(k_key_stats, dim3(grid_for(ctx, n, kBlock * 8, 1)), dim3(kBlock), 0, ctx->stream, kc, nullptr,
                               n, st.as<KeyStats>());
        } else {  // every partition in one launch
            KeySegs kss{};
            kss.ns = nparts;
            kss.gps = std::max(1, grid_for(ctx, n, kBlock * 8, 1) / nparts);
            for (int p = 0; p < nparts; ++p) kss.c[p] = make_colref(keys[p]), kss.n[p] = keys[p].length;
            hipLaunchKernelGGL(k_key_stats_segs, dim3(nparts * kss.gps), dim3(kBlock), 0, ctx->stream, kss, st.as<KeyStats>());
        }
    }
    QEH_TRY(read_small(ctx, &ks, st.p, sizeof ks));
    const bool any_valid = ks.mn <= ks.mx;
    const int64_t mn = any_valid ? ks.mn : 0, mx = any_valid ? ks.mx : 0;
    const uint64_t range = (uint64_t)mx - (uint64_t)mn;  // value codes 0 .. range (+ bias)
    const uint64_t bias = nullable && nulls_first ? 1 : 0;
    const uint64_t null_code = nullable && nulls_first ? 0 : range + 1;  // (no NULLs: never produced)
    // the largest code: range (+ 1 for the NULL code when nullable); a nullable key spanning the
    // whole Int64 range has no free code left, so it takes the permutation sort
    if (nullable && range == UINT64_MAX) return kPayloadSortNotEligible;
    const uint64_t max_code = range + (nullable ? 1 : 0);
    int bits = 1;
    while (bits < 64 && (max_code >> bits) != 0) ++bits;
    const int npass = (bits + kRadixBits - 1) / kRadixBits;
    // ping-pong buffers; pass 0 reads the payload column itself, the last pass writes the output
    // columns: the payload, and the key decoded from its codes (+ one valid byte per row when nullable)
    QEH_TRY(alloc_column(ctx, val.dtype, n, false, out_val));
    int s = alloc_column(ctx, key.dtype, n, nullable, out_key);
    if (s != QEH_OK) {
        qeh_column_release(ctx, out_val);
        return s;
    }
    DevBuf kb[2], vtmp, hist, offs, validb;
    const int nblocks = (int)std::min<int64_t>(std::max<int64_t>((n + kRsSTile - 1) / kRsSTile, 1), (int64_t)ctx->props.multiProcessorCount);
    const int64_t seg = (n + nblocks - 1) / nblocks;
    if (kb[0].alloc(ctx, n * 8) || kb[1].alloc(ctx, n * 8) || vtmp.alloc(ctx, n * 8) ||
        hist.alloc(ctx, (size_t)kRadix * nblocks * 4) || offs.alloc(ctx, (size_t)kRadix * nblocks * 8) ||
        (nullable && validb.alloc(ctx, n)))
        s = fail(QEH_E_OOM, "payload sort: out of device memory");
    // pass p reads buffer p % 2 (pass 0: the input column) and writes (p + 1) % 2
    const uint64_t *vsrc = (const uint64_t *)((const char *)val.values + (size_t)val.offset * 8);
    uint64_t *vb[2];
    vb[npass % 2] = (uint64_t *)out_val->values;
    vb[(npass + 1) % 2] = vtmp.as<uint64_t>();
    // pass 0 encodes the key column on load (histogram and scatter), the last pass decodes on store
    RsEncode enc{kc, mn, mx, bias, null_code, asc ? 1 : 0};
    auto segs = [&](RsEncode &e) {
        if (nparts == 1) return;
        e.ns = nparts;
        int64_t at = 0;
        for (int p = 0; p < nparts; ++p) {
            e.start[p] = at;
            e.sk[p] = make_colref(keys[p]);
            e.sv[p] = (const uint64_t *)((const char *)vals[p].values + (size_t)vals[p].offset * 8);
            at += keys[p].length;
        }
        e.start[nparts] = at;
    };
    segs(enc);
    const RsDecode dec{mn, mx, bias, null_code, asc ? 1 : 0, key.dtype, out_key->values, nullable ? validb.as<uint8_t>() : nullptr};
    const bool k32 = key.dtype == QEH_DT_INT32;
    // codes of 24..45 bits over many rows: the MSD passes (three passes over the rows); a sub-bucket
    // too large for its LDS sort sends the job on to the LSD passes below.  The NULL code gets a
    // sub-bucket (top 16 bits) of its own: the first one (NULLS FIRST: values biased past it) or the
    // one after the largest value's, so the NULLs are copied through instead of sharing an LDS sort.
    int mbits = 0;
    uint64_t mbias = 0, mnull = 0;
    if (s == QEH_OK && bits >= 24 && n >= ((int64_t)1 << 20) && !std::getenv("QEH_NO_MSD_SORT") &&
        range < (1ull << (kMsdBits + kMsdMaxLow))) {
        for (int bm = std::max(24, bits); bm <= kMsdBits + kMsdMaxLow && !mbits; ++bm) {
            const int s2 = bm - kMsdBits;
            const uint64_t top = range >> s2;  // the largest value's sub-bucket (unbiased)
            if (!nullable) mbits = bm;
            else if (top + 1 < (1ull << kMsdBits)) {
                mbits = bm;
                if (nulls_first) mbias = 1ull << s2, mnull = 0;
                else mnull = (top + 1) << s2;
            }
        }
    }
    bool done = false;
    if (mbits) {
        RsEncode encm{kc, mn, mx, mbias, mnull, asc ? 1 : 0};
        segs(encm);
        const RsDecode decm{mn, mx, mbias, mnull, asc ? 1 : 0, key.dtype, out_key->values, nullable ? validb.as<uint8_t>() : nullptr};
        const int r = msd_payload_passes(ctx, key, vsrc, n, mbits, encm, decm, kb[0].as<uint64_t>(), kb[1].as<uint64_t>(),
                                         vtmp.as<uint64_t>(), (uint64_t *)out_val->values);
        if (r == QEH_OK) done = true;
        else if (r != kMsdRedo) s = r;
    }
    for (int p = 0; p < npass && s == QEH_OK && !done; ++p) {
        KernelTimer kt(ctx, "radix_pass");
        const int c = p & 1, shift = p * kRadixBits;
        const bool first = p == 0, last = p + 1 == npass;
        if (first) {  // the key columns themselves, encoded on load
            auto hk = k32 ? k_rs_hist_enc<4> : k_rs_hist_enc<8>;
            hipLaunchKernelGGL(hk, dim3(nblocks), dim3(kRsThreads), 0, ctx->stream, n, seg, shift, hist.as<uint32_t>(), nblocks, enc);
        } else {
            hipLaunchKernelGGL((k_rs_hist<uint64_t, 0>), dim3(nblocks), dim3(kRsThreads), 0, ctx->stream, kb[c].as<uint64_t>(), n, seg,
                               shift, hist.as<uint32_t>(), nblocks, enc);
        }
        s = exclusive_scan_u32(ctx, hist.as<uint32_t>(), offs.as<uint64_t>(), (int64_t)kRadix * nblocks, nullptr);
        if (s != QEH_OK) break;
        const uint64_t *vin = first ? vsrc : vb[c];
        auto sk = first ? (last ? (k32 ? k_rs_scatter<uint64_t, true, uint64_t, true, 4> : k_rs_scatter<uint64_t, true, uint64_t, true, 8>)
                                : (k32 ? k_rs_scatter<uint64_t, true, uint64_t, false, 4> : k_rs_scatter<uint64_t, true, uint64_t, false, 8>))
                        : (last ? k_rs_scatter<uint64_t, true, uint64_t, true, 0> : k_rs_scatter<uint64_t, true, uint64_t, false, 0>);
        hipLaunchKernelGGL(sk, dim3(nblocks), dim3(kRsThreads), 0, ctx->stream, kb[c].as<uint64_t>(), vin, n, seg, shift,
                           offs.as<uint64_t>(), nblocks, kb[1 - c].as<uint64_t>(), vb[1 - c], nullptr, 0, dec, enc, nullptr);
        if (hipGetLastError() != hipSuccess) s = fail(QEH_E_HIP, "payload sort: pass launch failed");
    }
    if (s == QEH_OK && nullable) {
        KernelTimer kt(ctx, "sort_encode");
        hipLaunchKernelGGL(k_pack_valid, dim3(grid_for(ctx, (n + 63) / 64, kBlock, 8)), dim3(kBlock), 0, ctx->stream, validb.as<uint8_t>(),
                           n, (uint64_t *)out_key->validity);
        if (hipGetLastError() != hipSuccess) s = fail(QEH_E_HIP, "payload sort: validity launch failed");
    }
    if (s == QEH_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) s = fail(QEH_E_HIP, "payload sort failed");
    if (s != QEH_OK) {
        qeh_column_release(ctx, out_key);
        qeh_column_release(ctx, out_val);
        return s;
    }
    out_key->null_count = nullable ? -1 : 0;
    out_val->null_count = 0;
    return QEH_OK;
}

extern "C" int qeh_take(qeh_ctx *ctx, const qeh_column *col, const qeh_column *indices, qeh_column *out) {
    if (!ctx || !col || !indices || !out) return fail(QEH_E_INVALID, "qeh_take: bad argument");
    DeviceGuard dg(ctx->device);
    if (indices->validity) return fail(QEH_E_UNSUPPORTED, "take: nullable indices");
    const int64_t m = indices->length;
    if (indices->dtype == QEH_DT_UINT32) {
        const uint32_t *idx = (const uint32_t *)indices->values + indices->offset;
        QEH_TRY(gather_column(ctx, *col, idx, m, out));
        QEH_HIP(hipStreamSynchronize(ctx->stream));
        return QEH_OK;
    }
    if (indices->dtype != QEH_DT_INT64) return fail(QEH_E_INVALID, "take: indices must be UInt32 or Int64");
    DevBuf idx, bad;
    QEH_TRY(idx.alloc(ctx, (size_t)std::max<int64_t>(m, 1) * 4));
    QEH_TRY(bad.alloc(ctx, 8));
    QEH_HIP(hipMemsetAsync(bad.p, 0, 8, ctx->stream));
    if (m > 0)
        hipLaunchKernelGGL(k_u64_to_u32_idx, dim3(grid_for(ctx, m, kBlock * 8, 8)), dim3(kBlock), 0, ctx->stream,
                           (const int64_t *)indices->values + indices->offset, m, col->length, idx.as<uint32_t>(),
                           bad.as<uint32_t>());
    uint32_t b = 0;
    QEH_TRY(read_small(ctx, &b, bad.p, 4));
    if (b) return fail(QEH_E_INVALID, "take: index out of bounds");
    QEH_TRY(gather_column(ctx, *col, idx.as<uint32_t>(), m, out));
    QEH_HIP(hipStreamSynchronize(ctx->stream));
    return QEH_OK;
}

extern "C" int qeh_scatter(qeh_ctx *ctx, const qeh_column *col, const qeh_column *indices, qeh_column *out) {
    if (!ctx || !col || !indices || !out) return fail(QEH_E_INVALID, "qeh_scatter: bad argument");
    DeviceGuard dg(ctx->device);
    QEH_TRY(check_column(*col, "scatter"));
    if (indices->dtype != QEH_DT_UINT32 || indices->validity) return fail(QEH_E_INVALID, "scatter: indices must be non-null UInt32");
    if (indices->length != col->length) return fail(QEH_E_INVALID, "scatter: indices and column lengths differ");
    if (col->validity && col->null_count != 0) return fail(QEH_E_UNSUPPORTED, "scatter: nullable columns");
    int w = 0;
    switch (physical_dtype(col->dtype)) {
        case QEH_DT_INT64: case QEH_DT_FLOAT64: w = 8; break;
        case QEH_DT_INT32: case QEH_DT_FLOAT32: case QEH_DT_UINT32: w = 4; break;
        default: return fail(QEH_E_UNSUPPORTED, "scatter: fixed-width numeric columns only");
    }
    const int64_t m = col->length;
    QEH_TRY(alloc_column(ctx, col->dtype, m, false, out));
    if (m > 0) {
        KernelTimer kt(ctx, "scatter");
        const uint32_t *idx = (const uint32_t *)indices->values + indices->offset;
        const int grid = grid_for(ctx, m, kBlock * 8, 8);
        if (w == 8)
            hipLaunchKernelGGL(k_scatter<uint64_t>, dim3(grid), dim3(kBlock), 0, ctx->stream,
                               (const uint64_t *)col->values + col->offset, idx, m, (uint64_t *)out->values);
        else
            hipLaunchKernelGGL(k_scatter<uint32_t>, dim3(grid), dim3(kBlock), 0, ctx->stream,
                               (const uint32_t *)col->values + col->offset, idx, m, (uint32_t *)out->values);
    }
    QEH_HIP(hipGetLastError());
    QEH_HIP(hipStreamSynchronize(ctx->stream));
    return QEH_OK;
}
