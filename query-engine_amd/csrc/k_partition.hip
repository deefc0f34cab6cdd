// Partitioner / Exchange on the device: hash and range partition ids, the stable partition-major
// permutation (the radix passes of k_sort.hip over the ids), and the partition move that carries the
// payload columns in one pass instead of a permutation and gathers.
//
// Reference: hash partitioning follows Partitioner::partition_by_hash
// (crates/query-distributed/src/partition.rs:151-212) with a device hash; range partitioning
// find_range_partition (partition.rs:320-341).
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/qeh_plan.h"
#include "expr_device.h"
#include "fast_tile.h"
#include "radix_device.h"
#include "sort.h"

namespace qeh {

// Partition move (the device side of Exchange): one stable pass over u8 partition ids that
// carries up to 4 non-null 8-byte payload columns to their partition-major positions, with the
// same tile ranking and run-contiguous writes as k_rs_scatter — instead of a permutation
// followed by one gather per column (a gather re-reads every source line once per partition).
constexpr int kPmMaxCols = 4;
constexpr int kPmIpt = 4;
constexpr int kPmTile = kRsThreads * kPmIpt;  // 4096 rows: ids + 4 columns fit in LDS

struct PmCols {
    const uint64_t *src[kPmMaxCols];
    uint64_t *dst[kPmMaxCols];
    int32_t n;
};

// Rows whose id is >= `drop` (the filtered-out rows of a fused filter + exchange) are ranked last
// and not written.
template <int NC, bool AT = true>
__global__ __launch_bounds__(kRsThreads) void k_part_scatter(const uint8_t *__restrict__ ids, int64_t n, int64_t seg,
                                                             const uint64_t *__restrict__ offs, int nblocks, PmCols cols,
                                                             uint32_t drop) {
    constexpr int W = kRsThreads / 64;
    constexpr int DW = kRadix / 64;
    __shared__ uint64_t s_val[NC > 0 ? NC : 1][kPmTile];
    __shared__ uint8_t s_id[kPmTile];
    __shared__ uint32_t wcnt[W][kRadix];
    __shared__ uint32_t loc[kRadix];
    __shared__ uint32_t tot_s[kRadix];
    __shared__ uint32_t wsum[DW];
    __shared__ uint64_t run[kRadix];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    if (t < kRadix) run[t] = offs[(int64_t)t * nblocks + blockIdx.x];
    const int64_t lo = (int64_t)blockIdx.x * seg, hi = lo + seg < n ? lo + seg : n;
    // the next tile's ids and columns are loaded into registers while this tile is ranked, staged
    // and written (the barriers below order LDS only, so those loads stay in flight)
    uint32_t dgn[kPmIpt];
    uint64_t vn[kPmIpt][NC > 0 ? NC : 1];
    auto load = [&](int64_t c0) {
        const int64_t base = c0 + (int64_t)wave * 64 * kPmIpt + lane;
#pragma unroll
        for (int j = 0; j < kPmIpt; ++j) {
            const int64_t i = base + j * 64;
            const int64_t ii = i < hi ? i : hi - 1;
            dgn[j] = ids[ii];
#pragma unroll
            for (int c = 0; c < NC; ++c) vn[j][c] = __builtin_nontemporal_load(&cols.src[c][ii]);
        }
    };
    if (lo < hi) load(lo);
    __syncthreads();  // run[]
    for (int64_t c0 = lo; c0 < hi; c0 += kPmTile) {
        for (int i = t; i < W * kRadix; i += kRsThreads) (&wcnt[0][0])[i] = 0;
        const int64_t base = c0 + (int64_t)wave * 64 * kPmIpt + lane;
        uint32_t dg[kPmIpt];
        uint64_t v[kPmIpt][NC > 0 ? NC : 1];
#pragma unroll
        for (int j = 0; j < kPmIpt; ++j) {
            dg[j] = dgn[j];
#pragma unroll
            for (int c = 0; c < NC; ++c) v[j][c] = vn[j][c];
        }
        if (c0 + kPmTile < hi) load(c0 + kPmTile);
        lds_barrier();
        uint32_t rk[kPmIpt];
#pragma unroll
        for (int j = 0; j < kPmIpt; ++j) {
            const bool live = base + j * 64 < hi;
            rk[j] = tile_rank<AT>(wcnt[wave], dg[j], live);  // stable
        }
        lds_barrier();
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
        for (int j = 0; j < kPmIpt; ++j) {
            if (base + j * 64 < hi) {
                const uint32_t p = loc[dg[j]] + wcnt[wave][dg[j]] + rk[j];
                s_id[p] = (uint8_t)dg[j];
#pragma unroll
                for (int c = 0; c < NC; ++c) s_val[c][p] = v[j][c];
            }
        }
        lds_barrier();
        const int cnt = (int)(hi - c0 < kPmTile ? hi - c0 : kPmTile);
        for (int p = t; p < cnt; p += kRsThreads) {
            const uint32_t d = s_id[p];
            if (d >= drop) continue;
            const uint64_t pos = run[d] + (uint64_t)(p - (int)loc[d]);
#pragma unroll
            for (int c = 0; c < NC; ++c) cols.dst[c][pos] = s_val[c][p];
        }
        lds_barrier();
        if (t < kRadix) run[t] += tot_s[t];
    }
}

// k_part_scatter for at most kPsDig partitions (an Exchange to the GPUs of one node, config 4's 8):
// the same stable, run-contiguous placement with the bookkeeping sized to the partitions instead of
// 256 digits (16 per-wave counters, a 16-lane scan), 8192-row tiles for up to two columns, and rows
// with an id >= drop (the filtered-out rows) neither ranked nor staged, so the write loop covers only
// the rows that move.
template <int NC, bool AT = true>
__global__ __launch_bounds__(kRsThreads) void k_part_scatter_small(const uint8_t *__restrict__ ids, int64_t n, int64_t seg,
                                                                   const uint64_t *__restrict__ offs, int nblocks, PmCols cols,
                                                                   uint32_t drop) {
    constexpr int W = kRsThreads / 64;
    constexpr int IPT = NC <= 2 ? 8 : 4;
    constexpr int TILE = kRsThreads * IPT;
    __shared__ uint64_t s_val[NC > 0 ? NC : 1][TILE];
    __shared__ uint8_t s_id[TILE];
    __shared__ uint32_t wcnt[W][kPsDig];  // per-wave counts, then per-wave starts inside the partition
    __shared__ uint32_t loc[kPsDig], tot_s[kPsDig + 1];
    __shared__ uint64_t run[kPsDig];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    if (drop > (uint32_t)kPsDig) drop = kPsDig;
    if (t < kPsDig) run[t] = offs[(int64_t)t * nblocks + blockIdx.x];
    const int64_t lo = (int64_t)blockIdx.x * seg, hi = lo + seg < n ? lo + seg : n;
    uint32_t dgn[IPT];
    uint64_t vn[IPT][NC > 0 ? NC : 1];
    auto load = [&](int64_t c0) {
        const int64_t base = c0 + (int64_t)wave * 64 * IPT + lane;
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            const int64_t i = base + j * 64;
            const int64_t ii = i < hi ? i : hi - 1;
            dgn[j] = ids[ii];
#pragma unroll
            for (int c = 0; c < NC; ++c) vn[j][c] = __builtin_nontemporal_load(&cols.src[c][ii]);
        }
    };
    if (lo < hi) load(lo);
    __syncthreads();  // run[]
    for (int64_t c0 = lo; c0 < hi; c0 += TILE) {
        if (t < W * kPsDig) (&wcnt[0][0])[t] = 0u;
        const int64_t base = c0 + (int64_t)wave * 64 * IPT + lane;
        uint32_t dg[IPT];
        uint64_t v[IPT][NC > 0 ? NC : 1];
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            dg[j] = dgn[j];
#pragma unroll
            for (int c = 0; c < NC; ++c) v[j][c] = vn[j][c];
        }
        if (c0 + TILE < hi) load(c0 + TILE);
        lds_barrier();
        uint32_t rk[IPT];
        bool mv[IPT];
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            mv[j] = base + j * 64 < hi && dg[j] < drop;
            rk[j] = tile_rank<AT>(wcnt[wave], dg[j], mv[j]);  // stable
        }
        lds_barrier();
        if (t < 64) {  // lane d < kPsDig: per-wave starts inside partition d, its tile total, the scan
            uint32_t tot = 0;
            if (lane < kPsDig) {
#pragma unroll
                for (int w = 0; w < W; ++w) {
                    const uint32_t c = wcnt[w][lane];
                    wcnt[w][lane] = tot;
                    tot += c;
                }
            }
            const uint32_t incl = wave_incl_scan(tot);
            if (lane < kPsDig) loc[lane] = incl - tot, tot_s[lane] = tot;
            if (lane == kPsDig - 1) tot_s[kPsDig] = incl;  // rows that move in this tile
        }
        lds_barrier();
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            if (mv[j]) {
                const uint32_t p = loc[dg[j]] + wcnt[wave][dg[j]] + rk[j];
                s_id[p] = (uint8_t)dg[j];
#pragma unroll
                for (int c = 0; c < NC; ++c) s_val[c][p] = v[j][c];
            }
        }
        lds_barrier();
        const int cnt = (int)tot_s[kPsDig];
        for (int p = t; p < cnt; p += kRsThreads) {
            const uint32_t d = s_id[p];
            const uint64_t pos = run[d] + (uint64_t)(p - (int)loc[d]);
#pragma unroll
            for (int c = 0; c < NC; ++c) cols.dst[c][pos] = s_val[c][p];
        }
        lds_barrier();
        if (t < kPsDig) run[t] += tot_s[t];
    }
}

// The inverse of k_part_scatter_small (qeh_partition_hash_unmove): the same stable ranking of each
// tile's rows by partition, but every row reads its value from the partition-major column at the
// position the forward move gave it (run start + its rank in the partition) and writes it at its own
// input position.  A stable partition places row i at (rows of lower partitions) + (rows of its
// partition before i) whatever the tiling, so this reproduces any stable forward move.
template <int NC, bool AT = true>
__global__ __launch_bounds__(kRsThreads) void k_part_gather_small(const uint8_t *__restrict__ ids, int64_t n, int64_t seg,
                                                                  const uint64_t *__restrict__ offs, int nblocks, PmCols cols) {
    constexpr int W = kRsThreads / 64;
    constexpr int IPT = 8;
    constexpr int TILE = kRsThreads * IPT;
    __shared__ uint32_t wcnt[W][kPsDig];
    __shared__ uint32_t tot_s[kPsDig];
    __shared__ uint64_t run[kPsDig];
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63;
    if (t < kPsDig) run[t] = offs[(int64_t)t * nblocks + blockIdx.x];
    const int64_t lo = (int64_t)blockIdx.x * seg, hi = lo + seg < n ? lo + seg : n;
    __syncthreads();  // run[]
    for (int64_t c0 = lo; c0 < hi; c0 += TILE) {
        if (t < W * kPsDig) (&wcnt[0][0])[t] = 0u;
        const int64_t base = c0 + (int64_t)wave * 64 * IPT + lane;
        uint32_t dg[IPT];
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            const int64_t i = base + j * 64;
            dg[j] = ids[i < hi ? i : hi - 1];
        }
        lds_barrier();
        uint32_t rk[IPT];
        bool live[IPT];
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            live[j] = base + j * 64 < hi;
            rk[j] = tile_rank<AT>(wcnt[wave], dg[j], live[j]);  // stable, as the forward move
        }
        lds_barrier();
        if (t < kPsDig) {  // thread d: per-wave starts inside partition d, its tile total
            uint32_t tot = 0;
#pragma unroll
            for (int w = 0; w < W; ++w) {
                const uint32_t c = wcnt[w][t];
                wcnt[w][t] = tot;
                tot += c;
            }
            tot_s[t] = tot;
        }
        lds_barrier();
        uint64_t v[IPT][NC];
#pragma unroll
        for (int j = 0; j < IPT; ++j) {
            const uint64_t pos = live[j] ? run[dg[j]] + wcnt[wave][dg[j]] + rk[j] : 0;
#pragma unroll
            for (int c = 0; c < NC; ++c) v[j][c] = live[j] ? cols.src[c][pos] : 0;
        }
#pragma unroll
        for (int j = 0; j < IPT; ++j)
            if (live[j])
#pragma unroll
                for (int c = 0; c < NC; ++c) __builtin_nontemporal_store(v[j][c], &cols.dst[c][base + j * 64]);
        lds_barrier();
        if (t < kPsDig) run[t] += tot_s[t];
    }
}

// Filter + partition ids + per-segment histogram in one pass (config 4's probe side, fewer than
// kPsDig partitions): block b streams its segment [b * seg, (b + 1) * seg) -- seg a multiple of the
// 8192-row tile -- with FastTile's 16-B loads of the key and up to two term columns (every load of a
// tile issued before the predicate), writes the ids as u16 pairs and counts them per partition in
// byte-packed register counters, so no histogram pass re-reads the id stream.  The generic id pass
// (k_hash_ids8_pred) evaluated the predicate and loaded the key in two dependent rounds of 4-row
// loads (3.1 TB/s).  Rows past the last whole tile (the tail of the last segment) go row by row.
__device__ __forceinline__ uint32_t part_of_key(int64_t k, uint32_t parts) {
    uint64_t h = 0x9E3779B97F4A7C15ull;  // k_hash_ids8's hash of one non-null key column
    h = hash64(h ^ (hash64((uint64_t)k) + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2)));
    return (uint32_t)(h % parts);
}

template <int NTERMS>
__global__ __launch_bounds__(kRsThreads) void k_ids_hist_pred(FastIn in, PredTerms terms, int64_t n, int64_t seg,
                                                              uint32_t parts, uint8_t *__restrict__ ids,
                                                              uint32_t *__restrict__ hist, int nblocks) {
    constexpr int W = kRsThreads / 64, TILE = kRsThreads * kFastR;
    __shared__ uint32_t wc[W][kPsDig];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t lo = (int64_t)blockIdx.x * seg, hi = lo + seg < n ? lo + seg : n;
    const int64_t full = hi > lo ? lo + (hi - lo) / TILE * TILE : lo;
    uint32_t cnt[kPsDig];
#pragma unroll
    for (int d = 0; d < kPsDig; ++d) cnt[d] = 0u;
    uint64_t acc[2] = {0ull, 0ull};  // byte counters of partitions 0-7 / 8-15 (flushed before 256)
    auto flush = [&]() {
#pragma unroll
        for (int d = 0; d < kPsDig; ++d) cnt[d] += (uint32_t)(acc[d >> 3] >> (8 * (d & 7))) & 0xFFu;
        acc[0] = acc[1] = 0ull;
    };
    FastTile<NTERMS, 0, true> ft;
    int tiles = 0;
    if (lo < full) ft.issue(in, lo + (int64_t)wave * 512 + 2 * lane);
    for (int64_t t0 = lo; t0 < full; t0 += TILE) {
        ft.eval(in, terms);
        uint32_t id[kFastR];
#pragma unroll
        for (int r = 0; r < kFastR; ++r) id[r] = ((ft.sel >> r) & 1u) ? part_of_key(ft.k(r), parts) : parts;
        if (t0 + TILE < full) ft.issue(in, t0 + TILE + (int64_t)wave * 512 + 2 * lane);
        const int64_t base = t0 + (int64_t)wave * 512 + 2 * lane;
#pragma unroll
        for (int j = 0; j < kFastPairs; ++j) {
            *(uint16_t *)(ids + base + j * 128) = (uint16_t)(id[2 * j] | (id[2 * j + 1] << 8));
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const uint32_t d = id[2 * j + q];
                const uint64_t one = 1ull << (8 * (d & 7));
                acc[0] += d < 8 ? one : 0ull;
                acc[1] += d < 8 ? 0ull : one;
            }
        }
        if (++tiles == 31) {  // 31 tiles x 8 rows < 256 per byte counter
            flush();
            tiles = 0;
        }
    }
    flush();
    for (int64_t i = full + t; i < hi; i += kRsThreads) {  // ragged tail, one row per thread
        bool ok = NTERMS == 0 || !terms.is_or;
#pragma unroll
        for (int q = 0; q < NTERMS; ++q) {
            const PredTerm pt = terms.t[q];
            int64_t v = in.term[q][i];
            if (pt.ctype == QEH_DT_FLOAT64) v = f64_order_key(in.term_dt[q] == QEH_DT_FLOAT64 ? as_f64(v) : (double)v);
            const bool tr = cmp_i64(pt.op, v, pt.lit);
            ok = terms.is_or ? (q == 0 ? tr : (ok || tr)) : (ok && tr);
        }
        const uint32_t d = ok ? part_of_key(in.key[i], parts) : parts;
        ids[i] = (uint8_t)d;
#pragma unroll
        for (int e = 0; e < kPsDig; ++e) cnt[e] += d == (uint32_t)e ? 1u : 0u;
    }
#pragma unroll
    for (int d = 0; d < kPsDig; ++d) {
        uint32_t c = cnt[d];
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) c += __shfl_xor(c, o, 64);
        if (lane == 0) wc[wave][d] = c;
    }
    __syncthreads();
    if (t < kPsDig) {
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) c += wc[w][t];
        hist[(int64_t)t * nblocks + blockIdx.x] = c;  // digit-major, as k_rs_hist_u8
    }
}

// ---- hash partition ---------------------------------------------------------------------------
__global__ void k_partition_ids(ColRef key, int64_t n, uint32_t parts, uint64_t *__restrict__ keys,
                                uint32_t *__restrict__ idx) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t p = 0;  // NULL keys hash like an empty key (partition.rs:292-316 skips them)
        if (col_valid(key, i)) p = (uint32_t)(hash64((uint64_t)load_i64(key, i)) % parts);
        keys[i] = p;
        idx[i] = (uint32_t)i;
    }
}

// range partition: NULL -> 0 (NULLs sort first); value -> number of splitters
// strictly below (ascending) / above (descending) its order key, so equal keys
// share a partition and partition p precedes p+1 in sort order
__global__ void k_range_ids(ColRef key, int64_t n, const int64_t *__restrict__ split, int n_split, int asc,
                            uint64_t *__restrict__ keys, uint32_t *__restrict__ idx) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t p = 0;
        if (col_valid(key, i)) {
            const int64_t k = ordered_key(key, i);
            for (int j = 0; j < n_split; ++j) p += asc ? split[j] < k : split[j] > k;
        }
        keys[i] = p;
        idx[i] = (uint32_t)i;
    }
}

// ---- range partition by strings (qeh_range_partition_utf8) --------------------------------------
// k_range_ids for a Utf8 key against up to 255 splitter strings, in the byte-wise unsigned order of
// k_utf8_cmp and of the codes of qeh_utf8_dict_encode (a proper prefix before any longer string).
// Every workgroup keeps, per splitter, its first 8 bytes packed big-endian into one word (zero past
// the end; k_dict_pack's packing) and its byte range in LDS.  A row packs its own first 8 bytes the
// same way and binary-searches the words (at most 8 steps); only where the two words tie are more
// bytes compared: by length when either string ends inside the word, else 8 bytes at a time from
// byte 8 on.  The splitter bytes live in LDS when all of them fit kRpLdsBytes (LDS = true), else they
// are read from global memory (255 splitters of any length).  NULL rows read no bytes; one row per
// lane, no lane waits on another; every loop is bounded by the splitter count or a string's length.
constexpr int kRpMaxSplit = kRadix - 1;
constexpr int kRpLdsBytes = 16 * 1024;  // splitter bytes kept in LDS (+ 2 KiB words, 1 KiB offsets)

struct Utf8KeyIn {
    ColRef valid;         // validity only
    const int32_t *offs;  // advanced by the column offset
    const uint8_t *data;
};

// bytes [0, min(rem, 8)) at p as one big-endian word, zero past the end; reads no other byte
__device__ __forceinline__ uint64_t rp_word(const uint8_t *p, int32_t rem) {
    uint64_t w = 0;
    if (rem >= 8) {
        __builtin_memcpy(&w, p, 8);
    } else {
#pragma unroll
        for (int b = 0; b < 7; ++b)
            if (b < rem) w |= (uint64_t)p[b] << (8 * b);
    }
    return __builtin_bswap64(w);
}

// the order of splitter `sp` (sl bytes, first word sw) against the row `rp` (rl bytes, first word rw):
// < 0 splitter first, 0 equal, > 0 row first
__device__ __forceinline__ int rp_cmp(uint64_t sw, const uint8_t *sp, int32_t sl, uint64_t rw, const uint8_t *rp, int32_t rl) {
    if (sw != rw) return sw < rw ? -1 : 1;
    const int32_t m = sl < rl ? sl : rl;
    // equal words and a string that ends inside them: the common prefix is equal and the longer
    // string continues with 0x00 bytes only (inside the word), so the shorter one sorts first
    for (int32_t o = 8; o < m; o += 8) {
        const uint64_t a = rp_word(sp + o, m - o), b = rp_word(rp + o, m - o);
        if (a != b) return a < b ? -1 : 1;
    }
    return sl < rl ? -1 : (sl > rl ? 1 : 0);
}

template <bool LDS>
__global__ __launch_bounds__(kBlock) void k_range_ids_utf8(Utf8KeyIn key, int64_t n, const int32_t *__restrict__ sp_offs,
                                                           const uint8_t *__restrict__ sp_bytes, int n_split, int asc,
                                                           uint64_t *__restrict__ ids, uint32_t *__restrict__ idx) {
    __shared__ uint64_t s_word[kRpMaxSplit + 1];
    __shared__ int32_t s_off[kRpMaxSplit + 2];
    __shared__ uint32_t s_bytes[LDS ? kRpLdsBytes / 4 : 2];
    for (int j = threadIdx.x; j <= n_split; j += kBlock) s_off[j] = sp_offs[j];
    __syncthreads();
    for (int j = threadIdx.x; j < n_split; j += kBlock) s_word[j] = rp_word(sp_bytes + s_off[j], s_off[j + 1] - s_off[j]);
    if (LDS) {  // whole words: the host pads the device copy of the bytes to a multiple of 4 and checked the fit
        const int32_t words = ((s_off[n_split] < kRpLdsBytes ? s_off[n_split] : kRpLdsBytes) + 3) / 4;
        for (int32_t w = threadIdx.x; w < words; w += kBlock) s_bytes[w] = ((const uint32_t *)sp_bytes)[w];
    }
    __syncthreads();
    const uint8_t *sb = LDS ? (const uint8_t *)s_bytes : sp_bytes;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        uint32_t p = 0;  // NULL -> 0, as k_range_ids
        if (col_valid(key.valid, i)) {
            const int32_t s = key.offs[i], len = key.offs[i + 1] - s;
            const uint8_t *rp = key.data + s;
            const uint64_t rw = rp_word(rp, len);
            // ascending: the splitters strictly below the row = the first splitter >= it;
            // descending: the splitters strictly above it = n_split - the first splitter > it
            int lo = 0, hi = n_split;
            for (int step = 0; step < 8 && lo < hi; ++step) {  // 2^8 > kRpMaxSplit
                const int mid = (lo + hi) >> 1;
                const int c = rp_cmp(s_word[mid], sb + s_off[mid], s_off[mid + 1] - s_off[mid], rw, rp, len);
                if (asc ? c < 0 : c <= 0) lo = mid + 1;
                else hi = mid;
            }
            p = (uint32_t)(asc ? lo : n_split - lo);
        }
        ids[i] = p;
        idx[i] = (uint32_t)i;
    }
}

// PartitionStrategy::Hash over several key columns (partition.rs:151-212, compute_row_hash
// :292-316): NULL cells contribute nothing to the row hash, as the reference skips them; Int32 /
// Int64 values and Utf8 bytes are mixed into one 64-bit hash (the hash function is not
// observable in results).
struct HashKeys {
    ColRef c[kMaxCols];
    const int32_t *offs[kMaxCols];
    const uint8_t *data[kMaxCols];
    int32_t n;
};

__global__ void k_hash_ids_multi(HashKeys keys, int64_t n, uint32_t parts, uint64_t *__restrict__ ids,
                                 uint32_t *__restrict__ idx) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t h = 0x9E3779B97F4A7C15ull;
        for (int j = 0; j < keys.n; ++j) {
            const ColRef &c = keys.c[j];
            if (!col_valid(c, i)) continue;
            uint64_t v;
            if (c.dtype == QEH_DT_UTF8) {
                v = 0xcbf29ce484222325ull;  // FNV-1a over the bytes
                for (int32_t b = keys.offs[j][i]; b < keys.offs[j][i + 1]; ++b) v = (v ^ keys.data[j][b]) * 0x100000001b3ull;
            } else {
                v = (uint64_t)load_i64(c, i);
            }
            h = hash64(h ^ (hash64(v) + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2)));
        }
        ids[i] = h % parts;
        idx[i] = (uint32_t)i;
    }
}

__global__ void k_hash_ids8(HashKeys keys, int64_t n, uint32_t parts, uint8_t *__restrict__ ids) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        uint64_t h = 0x9E3779B97F4A7C15ull;
        for (int j = 0; j < keys.n; ++j) {
            const ColRef &c = keys.c[j];
            if (!col_valid(c, i)) continue;
            uint64_t v;
            if (c.dtype == QEH_DT_UTF8) {
                v = 0xcbf29ce484222325ull;
                for (int32_t b = keys.offs[j][i]; b < keys.offs[j][i + 1]; ++b) v = (v ^ keys.data[j][b]) * 0x100000001b3ull;
            } else {
                v = (uint64_t)load_i64(c, i);
            }
            h = hash64(h ^ (hash64(v) + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2)));
        }
        ids[i] = (uint8_t)(h % parts);
    }
}

// k_hash_ids8 for one non-null Int64 key column: eight rows per thread (four 16-B loads, one 8-B
// store of ids), the same hash.
__global__ __launch_bounds__(kBlock) void k_hash_ids8_i64(const int64_t *__restrict__ key, int64_t n, uint32_t parts,
                                                          uint8_t *__restrict__ ids) {
    typedef long long v2i64h __attribute__((ext_vector_type(2)));
    for (int64_t i0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * 8; i0 < n; i0 += (int64_t)gridDim.x * kBlock * 8) {
        uint64_t v[8];
        if (i0 + 8 <= n && (((uintptr_t)(key + i0)) & 15) == 0) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const v2i64h w = __builtin_nontemporal_load((const v2i64h *)(key + i0) + q);
                v[2 * q] = (uint64_t)w[0], v[2 * q + 1] = (uint64_t)w[1];
            }
        } else {
#pragma unroll
            for (int q = 0; q < 8; ++q) v[q] = i0 + q < n ? (uint64_t)key[i0 + q] : 0ull;
        }
        uint64_t out = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            uint64_t h = 0x9E3779B97F4A7C15ull;
            h = hash64(h ^ (hash64(v[q]) + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2)));
            out |= (uint64_t)(uint8_t)(h % parts) << (8 * q);
        }
        if (i0 + 8 <= n) {
            *(uint64_t *)(ids + i0) = out;
        } else {
            for (int q = 0; q < 8 && i0 + q < n; ++q) ids[i0 + q] = (uint8_t)(out >> (8 * q));
        }
    }
}

// The filter of a shuffle fused into the Exchange's id pass (config 4's probe side): rows whose
// predicate (an AND / OR list of column-literal comparisons) is TRUE get hash(key) % parts,
// the others `parts` (dropped by k_part_scatter).  One key column, Int32 / Int64.
__global__ __launch_bounds__(kBlock) void k_hash_ids8_pred(ColRef key, ColSet cols, PredTerms terms, int64_t n,
                                                           uint32_t parts, uint8_t *__restrict__ ids) {
    constexpr int R = 4;
    for (int64_t t0 = (int64_t)blockIdx.x * kBlock * R; t0 < n; t0 += (int64_t)gridDim.x * kBlock * R) {
        const int64_t row0 = t0 + threadIdx.x;
        const uint32_t m = eval_terms<R>(terms, cols, row0, kBlock, n);
        int64_t kv[R];
        uint32_t kvalid;
        load_rows<R>(key, row0, kBlock, n, kv, kvalid);
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t i = row0 + (int64_t)r * kBlock;
            if (i >= n) continue;
            uint64_t h = 0x9E3779B97F4A7C15ull;  // k_hash_ids8's hash of one key column (NULL skipped)
            if ((kvalid >> r) & 1u) h = hash64(h ^ (hash64((uint64_t)kv[r]) + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2)));
            ids[i] = ((m >> r) & 1u) ? (uint8_t)(h % parts) : (uint8_t)parts;
        }
    }
}

// PartitionStrategy::Range (find_range_partition, partition.rs:320-341): the first boundary the
// value is below, or len(boundaries); NULL -> 0; only Int64 keys are ranged (every other column
// type lands in partition 0, as in the reference)
__global__ void k_range_ids_first_below(ColRef key, int64_t n, const int64_t *__restrict__ b, int nb, int is_i64,
                                        uint64_t *__restrict__ ids, uint32_t *__restrict__ idx) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        uint32_t p = 0;
        if (is_i64 && col_valid(key, i)) {
            const int64_t v = ((const int64_t *)key.values)[i];
            p = (uint32_t)nb;
            for (int j = 0; j < nb; ++j)
                if (v < b[j]) {
                    p = (uint32_t)j;
                    break;
                }
        }
        ids[i] = p;
        idx[i] = (uint32_t)i;
    }
}

__global__ void k_count_parts(const uint64_t *__restrict__ ids, int64_t n, int parts, unsigned long long *__restrict__ counts) {
    __shared__ uint32_t h[kRadix];
    for (int i = threadIdx.x; i < kRadix; i += blockDim.x) h[i] = 0;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        atomicAdd(&h[ids[i]], 1u);
    __syncthreads();
    for (int p = threadIdx.x; p < parts; p += blockDim.x)
        if (h[p]) atomicAdd(&counts[p], (unsigned long long)h[p]);
}

}  // namespace qeh

using namespace qeh;

static int make_hash_keys(const qeh_column *keys, int n_keys, HashKeys *hk, int64_t *n) {
    hk->n = n_keys;
    *n = keys[0].length;
    for (int j = 0; j < n_keys; ++j) {
        QEH_TRY(check_column(keys[j], "partition key"));
        if (keys[j].length != *n) return fail(QEH_E_INVALID, "partition keys have different lengths");
        if (keys[j].dtype != QEH_DT_INT64 && keys[j].dtype != QEH_DT_INT32 && keys[j].dtype != QEH_DT_UTF8)
            return fail(QEH_E_UNSUPPORTED, "hash partition keys must be Int32 / Int64 / Utf8 (compute_row_hash)");
        hk->c[j] = make_colref(keys[j]);
        if (keys[j].dtype == QEH_DT_UTF8) {
            hk->offs[j] = keys[j].offsets + keys[j].offset;
            hk->data[j] = (const uint8_t *)keys[j].values;
        }
    }
    return QEH_OK;
}

// Stable partition-major permutation from per-row partition ids written by `ids`.
template <typename IdLaunch>
static int partition_perm(qeh_ctx *ctx, int64_t n, int n_parts, IdLaunch ids, const char *timer, int64_t *counts,
                          qeh_column *out_perm) {
    RadixState rs;
    rs.n = n;
    for (int b = 0; b < 2; ++b) {
        QEH_TRY(rs.k[b].alloc(ctx, (size_t)std::max<int64_t>(n, 1) * 8));
        QEH_TRY(rs.v[b].alloc(ctx, (size_t)std::max<int64_t>(n, 1) * 4));
    }
    std::fill(counts, counts + n_parts, 0);
    if (n > 0) {
        {
            KernelTimer kt(ctx, timer);
            ids(rs.k[0].as<uint64_t>(), rs.v[0].as<uint32_t>());
        }
        QEH_HIP(hipGetLastError());
        QEH_TRY(radix_passes(ctx, rs, n_parts > 1 ? bit_length((uint64_t)n_parts - 1) : 0));
    }
    QEH_TRY(alloc_column(ctx, QEH_DT_UINT32, n, false, out_perm));
    if (n > 0) {
        QEH_HIP(hipMemcpyAsync(out_perm->values, rs.v[rs.cur].p, (size_t)n * 4, hipMemcpyDeviceToDevice, ctx->stream));
        DevBuf cnt;
        int s = cnt.alloc(ctx, (size_t)n_parts * 8);
        if (s == QEH_OK) {
            QEH_HIP(hipMemsetAsync(cnt.p, 0, (size_t)n_parts * 8, ctx->stream));
            hipLaunchKernelGGL(k_count_parts, dim3(grid_for(ctx, n, kBlock * 16, 4)), dim3(kBlock), 0, ctx->stream,
                               rs.k[rs.cur].as<uint64_t>(), n, n_parts, cnt.as<unsigned long long>());
            s = read_small(ctx, counts, cnt.p, (size_t)n_parts * 8);
        }
        if (s != QEH_OK) {
            qeh_column_release(ctx, out_perm);
            return s;
        }
    }
    QEH_HIP(hipStreamSynchronize(ctx->stream));
    return QEH_OK;
}

extern "C" int qeh_hash_partition(qeh_ctx *ctx, const qeh_column *key, int n_parts, int64_t *counts,
                                  qeh_column *out_perm) {
    if (!ctx || !key || !counts || !out_perm || n_parts < 1 || n_parts > kRadix)
        return fail(QEH_E_INVALID, "qeh_hash_partition: bad argument (1..256 partitions)");
    DeviceGuard dg(ctx->device);
    QEH_TRY(check_column(*key, "partition key"));
    if (key->dtype != QEH_DT_INT64 && key->dtype != QEH_DT_INT32)
        return fail(QEH_E_UNSUPPORTED, "partition keys must be Int32/Int64 on the device");
    const int64_t n = key->length;
    const ColRef kc = make_colref(*key);
    return partition_perm(
        ctx, n, n_parts,
        [&](uint64_t *ids, uint32_t *idx) {
            hipLaunchKernelGGL(k_partition_ids, dim3(grid_for(ctx, n, kBlock * 8, 8)), dim3(kBlock), 0, ctx->stream, kc,
                               n, (uint32_t)n_parts, ids, idx);
        },
        "hash_partition", counts, out_perm);
}

extern "C" int qeh_range_partition(qeh_ctx *ctx, const qeh_column *key, int ascending, const int64_t *splitters,
                                   int n_splitters, int64_t *counts, qeh_column *out_perm) {
    if (!ctx || !key || !counts || !out_perm || n_splitters < 0 || n_splitters >= kRadix ||
        (n_splitters > 0 && !splitters))
        return fail(QEH_E_INVALID, "qeh_range_partition: bad argument (0..255 splitters)");
    DeviceGuard dg(ctx->device);
    QEH_TRY(check_column(*key, "partition key"));
    if (key->dtype == QEH_DT_UTF8) return fail(QEH_E_UNSUPPORTED, "Utf8 range partition keys are not supported on the device");
    if (is_temporal(key->dtype)) return fail(QEH_E_UNSUPPORTED, "temporal range partition keys are not supported on the device");
    for (int j = 1; j < n_splitters; ++j)
        if (splitters[j] < splitters[j - 1]) return fail(QEH_E_INVALID, "qeh_range_partition: splitters must be ascending");
    const int64_t n = key->length;
    DevBuf sp;
    QEH_TRY(sp.alloc(ctx, (size_t)std::max(n_splitters, 1) * 8));
    if (n_splitters > 0)
        QEH_HIP(hipMemcpyAsync(sp.p, splitters, (size_t)n_splitters * 8, hipMemcpyHostToDevice, ctx->stream));
    QEH_HIP(hipStreamSynchronize(ctx->stream));  // host splitter array may go away
    const ColRef kc = make_colref(*key);
    return partition_perm(
        ctx, n, n_splitters + 1,
        [&](uint64_t *ids, uint32_t *idx) {
            hipLaunchKernelGGL(k_range_ids, dim3(grid_for(ctx, n, kBlock * 8, 8)), dim3(kBlock), 0, ctx->stream, kc, n,
                               sp.as<int64_t>(), n_splitters, ascending ? 1 : 0, ids, idx);
        },
        "range_partition", counts, out_perm);
}

extern "C" int qeh_range_partition_utf8(qeh_ctx *ctx, const qeh_column *key, int ascending, const int32_t *splitter_offsets,
                                        const uint8_t *splitter_bytes, int n_splitters, int64_t *counts,
                                        qeh_column *out_perm) {
    if (!ctx || !key || !counts || !out_perm || !splitter_offsets || n_splitters < 0 || n_splitters > kRpMaxSplit)
        return fail(QEH_E_INVALID, "qeh_range_partition_utf8: bad argument (0..255 splitters)");
    if (splitter_offsets[0] != 0) return fail(QEH_E_INVALID, "qeh_range_partition_utf8: splitter offsets must start at 0");
    for (int j = 0; j < n_splitters; ++j)
        if (splitter_offsets[j + 1] < splitter_offsets[j])
            return fail(QEH_E_INVALID, "qeh_range_partition_utf8: splitter offsets must not decrease");
    const int32_t total = splitter_offsets[n_splitters];
    if (total > 0 && !splitter_bytes) return fail(QEH_E_INVALID, "qeh_range_partition_utf8: bad argument (no splitter bytes)");
    for (int j = 1; j < n_splitters; ++j) {  // byte-wise unsigned, a proper prefix first
        const int32_t a = splitter_offsets[j - 1], b = splitter_offsets[j], c = splitter_offsets[j + 1];
        const int32_t la = b - a, lb = c - b, m = std::min(la, lb);
        const int d = m > 0 ? std::memcmp(splitter_bytes + a, splitter_bytes + b, (size_t)m) : 0;
        if (d > 0 || (d == 0 && la > lb))
            return fail(QEH_E_INVALID, "qeh_range_partition_utf8: splitters must be ascending");
    }
    DeviceGuard dg(ctx->device);
    QEH_TRY(check_column(*key, "partition key"));
    if (key->dtype != QEH_DT_UTF8)
        return fail(QEH_E_UNSUPPORTED, "qeh_range_partition_utf8: the key must be Utf8 (qeh_range_partition takes the other types)");
    const int64_t n = key->length;
    if (n > 0 && !key->offsets) return fail(QEH_E_INVALID, "partition key: null offsets pointer");
    DevBuf so, sb;
    QEH_TRY(so.alloc(ctx, (size_t)(n_splitters + 1) * 4));
    QEH_TRY(sb.alloc(ctx, (size_t)total + 8));  // (whole words past the end for the copy into LDS)
    QEH_HIP(hipMemcpyAsync(so.p, splitter_offsets, (size_t)(n_splitters + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    if (total > 0) QEH_HIP(hipMemcpyAsync(sb.p, splitter_bytes, (size_t)total, hipMemcpyHostToDevice, ctx->stream));
    QEH_HIP(hipStreamSynchronize(ctx->stream));  // the host splitter arrays may go away
    Utf8KeyIn in{};
    in.valid = make_colref(*key);
    in.offs = key->offsets + key->offset;
    in.data = (const uint8_t *)key->values;
    const bool lds = total <= kRpLdsBytes;
    return partition_perm(
        ctx, n, n_splitters + 1,
        [&](uint64_t *ids, uint32_t *idx) {
            hipLaunchKernelGGL(lds ? k_range_ids_utf8<true> : k_range_ids_utf8<false>, dim3(grid_for(ctx, n, kBlock * 4, 8)),
                               dim3(kBlock), 0, ctx->stream, in, n, so.as<int32_t>(), sb.as<uint8_t>(), n_splitters,
                               ascending ? 1 : 0, ids, idx);
        },
        "range_partition_utf8", counts, out_perm);
}

extern "C" int qeh_partition_hash(qeh_ctx *ctx, const qeh_column *keys, int n_keys, int n_parts, int64_t *counts,
                                  qeh_column *out_perm) {
    if (!ctx || !keys || n_keys < 1 || n_keys > kMaxCols || !counts || !out_perm || n_parts < 1 || n_parts > kRadix)
        return fail(QEH_E_INVALID, "qeh_partition_hash: bad argument (1..12 keys, 1..256 partitions)");
    DeviceGuard dg(ctx->device);
    HashKeys hk{};
    int64_t n;
    QEH_TRY(make_hash_keys(keys, n_keys, &hk, &n));
    return partition_perm(
        ctx, n, n_parts,
        [&](uint64_t *ids, uint32_t *idx) {
            hipLaunchKernelGGL(k_hash_ids_multi, dim3(grid_for(ctx, n, kBlock * 8, 8)), dim3(kBlock), 0, ctx->stream, hk, n,
                               (uint32_t)n_parts, ids, idx);
        },
        "hash_partition", counts, out_perm);
}

// qeh_partition_hash_unmove: out_cols[c][i] = moved[c][position of row i in the stable partition-major
// order of qeh_partition_hash_move over the same key] -- the reverse of an Exchange's move, for results
// computed on the partition-major rows (distributed window functions return them into input order).
extern "C" int qeh_partition_hash_unmove(qeh_ctx *ctx, const qeh_column *key, int n_parts, const qeh_column *moved,
                                         int n_cols, qeh_column *out_cols) {
    if (!ctx || !key || !moved || !out_cols || n_cols < 1 || n_cols > 2 || n_parts < 1 || n_parts > kPsDig)
        return fail(QEH_E_INVALID, "qeh_partition_hash_unmove: bad argument (1..2 columns, 1..16 partitions)");
    DeviceGuard dg(ctx->device);
    const int64_t n = key->length;
    QEH_TRY(check_column(*key, "partition key"));
    if (key->dtype != QEH_DT_INT64 || (key->validity && key->null_count != 0) ||
        (((uintptr_t)key->values + (uintptr_t)key->offset * 8) & 15) != 0)
        return fail(QEH_E_UNSUPPORTED, "qeh_partition_hash_unmove: one non-null, 16-B aligned Int64 key");
    for (int c = 0; c < n_cols; ++c) {
        QEH_TRY(check_column(moved[c], "moved column"));
        if (moved[c].length != n || (moved[c].dtype != QEH_DT_INT64 && moved[c].dtype != QEH_DT_FLOAT64) ||
            (moved[c].validity && moved[c].null_count != 0))
            return fail(QEH_E_UNSUPPORTED, "qeh_partition_hash_unmove: non-null Int64 / Float64 columns of the key's length");
    }
    constexpr int64_t kFusedTile = (int64_t)kRsThreads * kFastR;
    int nblocks = (int)std::min<int64_t>(std::max<int64_t>((n + kFusedTile - 1) / kFusedTile, 1), (int64_t)ctx->props.multiProcessorCount);
    int64_t seg = (n + nblocks - 1) / nblocks;
    seg = std::max<int64_t>((seg + kFusedTile - 1) / kFusedTile * kFusedTile, kFusedTile);
    nblocks = (int)std::max<int64_t>((n + seg - 1) / seg, 1);
    int made = 0, s = QEH_OK;
    for (; made < n_cols; ++made)
        if ((s = alloc_column(ctx, moved[made].dtype, n, false, &out_cols[made])) != QEH_OK) break;
    if (s == QEH_OK && n > 0) {
        DevBuf ids, hist, offs;
        if (ids.alloc(ctx, (size_t)n) || hist.alloc(ctx, (size_t)kPsDig * nblocks * 4) ||
            offs.alloc(ctx, (size_t)kPsDig * nblocks * 8))
            s = fail(QEH_E_OOM, "partition unmove: out of device memory");
        KernelTimer kt(ctx, "partition_move");
        if (s == QEH_OK) {
            FastIn fin{};
            fin.key = (const int64_t *)key->values + key->offset;
            hipLaunchKernelGGL(k_ids_hist_pred<0>, dim3(nblocks), dim3(kRsThreads), 0, ctx->stream, fin, PredTerms{}, n, seg,
                               (uint32_t)n_parts, ids.as<uint8_t>(), hist.as<uint32_t>(), nblocks);
            s = exclusive_scan_u32(ctx, hist.as<uint32_t>(), offs.as<uint64_t>(), (int64_t)kPsDig * nblocks, nullptr);
        }
        if (s == QEH_OK) {
            PmCols pc{};
            pc.n = n_cols;
            for (int c = 0; c < n_cols; ++c) {
                pc.src[c] = (const uint64_t *)moved[c].values + moved[c].offset;
                pc.dst[c] = (uint64_t *)out_cols[c].values;
            }
            const bool ballot = rs_ballot(ctx);
            auto kf = n_cols == 1 ? (ballot ? k_part_gather_small<1, false> : k_part_gather_small<1, true>)
                                  : (ballot ? k_part_gather_small<2, false> : k_part_gather_small<2, true>);
            hipLaunchKernelGGL(kf, dim3(nblocks), dim3(kRsThreads), 0, ctx->stream, ids.as<uint8_t>(), n, seg,
                               offs.as<uint64_t>(), nblocks, pc);
            if (hipGetLastError() != hipSuccess) s = fail(QEH_E_HIP, "partition unmove launch failed");
        }
        if (s == QEH_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) s = fail(QEH_E_HIP, "partition unmove failed");
    }
    if (s != QEH_OK)
        for (int c = 0; c < made; ++c) qeh_column_release(ctx, &out_cols[c]);
    return s;
}

// ---- the partition move (qeh_partition_hash_move, qeh_filter_partition_hash_move) -----------------
// The segments of a move over n rows, one workgroup each.  fused: the ids come from the one-pass id +
// histogram kernel (k_ids_hist_pred), so segments are whole 8192-row tiles (16-B aligned pairs in
// every segment) and the histogram holds kPsDig digits instead of kRadix (digit-major).
struct MoveGrid {
    int nblocks;
    int64_t seg;
    bool fused;
    int ndig;
};

static MoveGrid move_grid(qeh_ctx *ctx, int64_t n, bool fused) {
    constexpr int64_t kFusedTile = (int64_t)kRsThreads * kFastR;
    MoveGrid g{};
    g.fused = fused;
    g.ndig = fused ? kPsDig : kRadix;
    g.nblocks = (int)std::min<int64_t>(std::max<int64_t>((n + kPmTile - 1) / kPmTile, 1), (int64_t)ctx->props.multiProcessorCount);
    g.seg = (n + g.nblocks - 1) / g.nblocks;
    if (fused) {
        g.seg = std::max<int64_t>((g.seg + kFusedTile - 1) / kFusedTile * kFusedTile, kFusedTile);
        g.nblocks = (int)std::max<int64_t>((n + g.seg - 1) / g.seg, 1);
    }
    return g;
}

// counts[p] += partition p's rows over every segment of the histogram (one synchronous read)
static int counts_from_hist(qeh_ctx *ctx, const DevBuf &hist, const MoveGrid &g, int n_parts, int64_t *counts) {
    std::vector<uint32_t> h((size_t)g.ndig * g.nblocks, 0);
    QEH_TRY(read_small(ctx, h.data(), hist.p, h.size() * 4));
    for (int p = 0; p < n_parts; ++p)
        for (int b = 0; b < g.nblocks; ++b) counts[p] += h[(size_t)p * g.nblocks + b];
    return QEH_OK;
}

// the nc moved columns: cols[src_idx[q]] -> out_cols[dst_idx[q]] (dst_idx == nullptr: out_cols[q])
static PmCols pack_pm_cols(const qeh_column *cols, const int32_t *src_idx, qeh_column *out_cols, const int32_t *dst_idx, int nc) {
    PmCols pc{};
    pc.n = nc;
    for (int q = 0; q < nc; ++q) {
        const qeh_column &src = cols[src_idx[q]];
        pc.src[q] = (const uint64_t *)src.values + src.offset;
        pc.dst[q] = (uint64_t *)out_cols[dst_idx ? dst_idx[q] : q].values;
    }
    return pc;
}

using PartScatterFn = void (*)(const uint8_t *, int64_t, int64_t, const uint64_t *, int, PmCols, uint32_t);
template <int NC>
static PartScatterFn part_scatter_fn(bool small, bool ballot) {
    if (small) return ballot ? k_part_scatter_small<NC, false> : k_part_scatter_small<NC, true>;
    return ballot ? k_part_scatter<NC, false> : k_part_scatter<NC, true>;
}

// One scatter of nc (1..kPmMaxCols) columns; rows with an id >= drop_id are left out.  small: the
// kernel for at most kPsDig partitions; ballot: rank by ballot peers (rs_ballot).
static void launch_part_scatter(qeh_ctx *ctx, int nc, bool small, bool ballot, const uint8_t *ids, int64_t n, int64_t seg,
                                const uint64_t *offs, int nblocks, const PmCols &pc, uint32_t drop_id) {
    PartScatterFn f;
    switch (nc) {
        case 1: f = part_scatter_fn<1>(small, ballot); break;
        case 2: f = part_scatter_fn<2>(small, ballot); break;
        case 3: f = part_scatter_fn<3>(small, ballot); break;
        default: f = part_scatter_fn<4>(small, ballot); break;
    }
    hipLaunchKernelGGL(f, dim3(nblocks), dim3(kRsThreads), 0, ctx->stream, ids, n, seg, offs, nblocks, pc, drop_id);
}

// Exchange's device side in one pass: partition ids, per-segment histograms, then the payload
// columns moved to partition-major order (k_part_scatter).  Columns that are not non-null
// 8-byte go through the permutation + gather path.
extern "C" int qeh_partition_hash_move(qeh_ctx *ctx, const qeh_column *keys, int n_keys, int n_parts,
                                       const qeh_column *cols, int n_cols, int64_t *counts, qeh_column *out_cols) {
    if (!ctx || !keys || n_keys < 1 || n_keys > kMaxCols || !counts || n_parts < 1 || n_parts > kRadix || n_cols < 0 ||
        (n_cols > 0 && (!cols || !out_cols)))
        return fail(QEH_E_INVALID, "qeh_partition_hash_move: bad argument (1..12 keys, 1..256 partitions)");
    DeviceGuard dg(ctx->device);
    HashKeys hk{};
    int64_t n;
    QEH_TRY(make_hash_keys(keys, n_keys, &hk, &n));
    for (int c = 0; c < n_cols; ++c) {
        QEH_TRY(check_column(cols[c], "partition column"));
        if (cols[c].length != n) return fail(QEH_E_INVALID, "partition columns and keys have different lengths");
    }
    auto movable = [](const qeh_column &c) {  // 8-byte values (Date64 / timestamps are Int64), moved as they are
        const int pt = physical_dtype(c.dtype);
        return (pt == QEH_DT_INT64 || pt == QEH_DT_FLOAT64) && (!c.validity || c.null_count == 0);
    };
    std::vector<int32_t> mv, other;
    for (int c = 0; c < n_cols; ++c) (movable(cols[c]) ? mv : other).push_back(c);
    std::fill(counts, counts + n_parts, 0);
    std::vector<char> made(n_cols, 0);
    auto cleanup = [&]() {
        for (int c = 0; c < n_cols; ++c)
            if (made[c]) qeh_column_release(ctx, &out_cols[c]);
    };
    // one non-null, 16-B aligned Int64 key into at most kPsDig partitions: ids and per-segment
    // histograms in one pass (k_ids_hist_pred without terms), segments of whole 8192-row tiles
    const qeh_column &k0 = keys[0];
    const bool fused = n_keys == 1 && n_parts <= kPsDig && k0.dtype == QEH_DT_INT64 &&
                       (!k0.validity || k0.null_count == 0) &&
                       (((uintptr_t)k0.values + (uintptr_t)k0.offset * 8) & 15) == 0 && !std::getenv("QEH_PM_GENERIC");
    const MoveGrid g = move_grid(ctx, n, fused);
    DevBuf ids, hist, offs;
    QEH_TRY(ids.alloc(ctx, (size_t)std::max<int64_t>(n, 1)));
    QEH_TRY(hist.alloc(ctx, (size_t)kRadix * g.nblocks * 4));
    QEH_TRY(offs.alloc(ctx, (size_t)kRadix * g.nblocks * 8));
    if (n > 0) {
        KernelTimer kt(ctx, "partition_move");
        if (fused) {
            FastIn fin{};
            fin.key = (const int64_t *)k0.values + k0.offset;
            hipLaunchKernelGGL(k_ids_hist_pred<0>, dim3(g.nblocks), dim3(kRsThreads), 0, ctx->stream, fin, PredTerms{}, n,
                               g.seg, (uint32_t)n_parts, ids.as<uint8_t>(), hist.as<uint32_t>(), g.nblocks);
        } else {
            if (n_keys == 1 && k0.dtype == QEH_DT_INT64 && (!k0.validity || k0.null_count == 0))
                hipLaunchKernelGGL(k_hash_ids8_i64, dim3(grid_for(ctx, (n + 7) / 8, kBlock, 8)), dim3(kBlock), 0,
                                   ctx->stream, (const int64_t *)k0.values + k0.offset, n, (uint32_t)n_parts,
                                   ids.as<uint8_t>());
            else
                hipLaunchKernelGGL(k_hash_ids8, dim3(grid_for(ctx, n, kBlock * 8, 8)), dim3(kBlock), 0, ctx->stream, hk, n,
                                   (uint32_t)n_parts, ids.as<uint8_t>());
            launch_hist_u8(ctx, ids.as<uint8_t>(), n, g.seg, hist.as<uint32_t>(), g.nblocks);  // ids are a byte stream: 16 per load
        }
        QEH_HIP(hipGetLastError());
        QEH_TRY(exclusive_scan_u32(ctx, hist.as<uint32_t>(), offs.as<uint64_t>(), (int64_t)g.ndig * g.nblocks, nullptr));
        QEH_TRY(counts_from_hist(ctx, hist, g, n_parts, counts));
    }
    int s = QEH_OK;
    for (int c : mv) {
        if ((s = alloc_column(ctx, cols[c].dtype, n, false, &out_cols[c])) != QEH_OK) break;
        made[c] = 1;
    }
    const bool small = n_parts <= kPsDig && !std::getenv("QEH_PM_GENERIC");
    for (size_t at = 0; s == QEH_OK && at < mv.size() && n > 0; at += kPmMaxCols) {
        const int nc = (int)std::min<size_t>(kPmMaxCols, mv.size() - at);
        const PmCols pc = pack_pm_cols(cols, mv.data() + at, out_cols, mv.data() + at, nc);
        KernelTimer kt(ctx, "partition_move");
        launch_part_scatter(ctx, nc, small, rs_ballot(ctx), ids.as<uint8_t>(), n, g.seg, offs.as<uint64_t>(), g.nblocks, pc,
                            (uint32_t)kRadix);
        if (hipGetLastError() != hipSuccess) s = fail(QEH_E_HIP, "partition move launch failed");
    }
    if (s == QEH_OK && !other.empty()) {  // permutation + gathers for the rest
        int64_t c2[kRadix];
        qeh_column perm{};
        s = qeh_partition_hash(ctx, keys, n_keys, n_parts, c2, &perm);
        for (size_t q = 0; s == QEH_OK && q < other.size(); ++q) {
            s = gather_column(ctx, cols[other[q]], (const uint32_t *)perm.values, n, &out_cols[other[q]]);
            if (s == QEH_OK) made[other[q]] = 1;
        }
        if (perm.owned) {
            (void)hipStreamSynchronize(ctx->stream);
            qeh_column_release(ctx, &perm);
        }
    }
    if (s == QEH_OK) {
        hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) s = fail(QEH_E_HIP, std::string("partition move: ") + hipGetErrorString(e));
    }
    if (s != QEH_OK) cleanup();
    return s;
}

// Filter + Exchange device side in two passes over the probe columns: partition ids of the
// qualifying rows (k_hash_ids8_pred), per-segment histograms, then the moved columns written
// partition-major with the rejected rows left out (k_part_scatter with a drop id).
extern "C" int qeh_filter_partition_hash_move(qeh_ctx *ctx, const qeh_column *cols, int n_cols, const qeh_expr *predicate,
                                              int key_idx, int n_parts, const int32_t *move_idx, int n_move,
                                              int64_t *counts, qeh_column *out_cols) {
    if (!ctx || !cols || n_cols < 1 || n_cols > kMaxCols || !predicate || key_idx < 0 || key_idx >= n_cols || !counts ||
        n_parts < 1 || n_parts >= kRadix || n_move < 1 || n_move > kPmMaxCols || !move_idx || !out_cols)
        return fail(QEH_E_INVALID, "qeh_filter_partition_hash_move: bad argument (1..255 partitions, 1..4 moved columns)");
    DeviceGuard dg(ctx->device);
    const int64_t n = cols[0].length;
    for (int c = 0; c < n_cols; ++c) {
        QEH_TRY(check_column(cols[c], "filter-partition column"));
        if (cols[c].length != n) return fail(QEH_E_INVALID, "filter-partition columns have different lengths");
    }
    const qeh_column &kc = cols[key_idx];
    if (kc.dtype != QEH_DT_INT64 && kc.dtype != QEH_DT_INT32)
        return fail(QEH_E_UNSUPPORTED, "qeh_filter_partition_hash_move: the key must be Int32 / Int64");
    for (int q = 0; q < n_move; ++q) {
        if (move_idx[q] < 0 || move_idx[q] >= n_cols) return fail(QEH_E_INVALID, "moved column index out of range");
        const qeh_column &c = cols[move_idx[q]];
        if ((c.dtype != QEH_DT_INT64 && c.dtype != QEH_DT_FLOAT64) || (c.validity && c.null_count != 0))
            return fail(QEH_E_UNSUPPORTED, "qeh_filter_partition_hash_move: moved columns must be non-null Int64 / Float64");
    }
    std::vector<int32_t> dts(n_cols);
    for (int i = 0; i < n_cols; ++i) dts[i] = cols[i].dtype;
    DevProgram prog;
    QEH_TRY(compile_expr(predicate, dts.data(), n_cols, &prog));
    if (prog.result_type != QEH_DT_BOOL) return fail(QEH_E_TYPE, "Filter predicate must return boolean");
    PredTerms terms{};
    if (!lower_to_terms(predicate, dts.data(), n_cols, &terms))
        return fail(QEH_E_UNSUPPORTED, "qeh_filter_partition_hash_move: predicate is not a list of column-literal comparisons");
    ColSet cs;
    QEH_TRY(make_colset(cols, n_cols, &cs));
    std::fill(counts, counts + n_parts, 0);
    // the fused id + histogram pass: fewer than kPsDig partitions, a non-null Int64 key and term
    // columns that are non-null 8-byte, 16-B aligned (FastTile's loads)
    auto fast_ok = [](const qeh_column &c) {
        return (c.dtype == QEH_DT_INT64 || c.dtype == QEH_DT_FLOAT64) && (!c.validity || c.null_count == 0) &&
               (((uintptr_t)c.values + (uintptr_t)c.offset * 8) & 15) == 0;
    };
    bool fused = n_parts < kPsDig && kc.dtype == QEH_DT_INT64 && fast_ok(kc) && terms.n <= 2 &&
                 !std::getenv("QEH_PM_GENERIC");
    FastIn fin{};
    if (fused) {
        fin.key = (const int64_t *)kc.values + kc.offset;
        for (int i = 0; i < terms.n; ++i) {
            const qeh_column &tc = cols[terms.t[i].col];
            if (!fast_ok(tc)) fused = false;
            fin.term[i] = (const int64_t *)tc.values + tc.offset;
            fin.term_dt[i] = tc.dtype;
        }
    }
    const MoveGrid g = move_grid(ctx, n, fused);
    DevBuf ids, hist, offs;
    QEH_TRY(ids.alloc(ctx, (size_t)std::max<int64_t>(n, 1)));
    QEH_TRY(hist.alloc(ctx, (size_t)kRadix * g.nblocks * 4));
    QEH_TRY(offs.alloc(ctx, (size_t)kRadix * g.nblocks * 8));
    int64_t kept = 0;
    if (n > 0) {
        KernelTimer kt(ctx, "partition_move");
        if (fused) {
            auto ih = terms.n == 0 ? k_ids_hist_pred<0> : terms.n == 1 ? k_ids_hist_pred<1> : k_ids_hist_pred<2>;
            hipLaunchKernelGGL(ih, dim3(g.nblocks), dim3(kRsThreads), 0, ctx->stream, fin, terms, n, g.seg, (uint32_t)n_parts,
                               ids.as<uint8_t>(), hist.as<uint32_t>(), g.nblocks);
        } else {
            hipLaunchKernelGGL(k_hash_ids8_pred, dim3(grid_for(ctx, n, kBlock * 4, 8)), dim3(kBlock), 0, ctx->stream,
                               make_colref(kc), cs, terms, n, (uint32_t)n_parts, ids.as<uint8_t>());
            launch_hist_u8(ctx, ids.as<uint8_t>(), n, g.seg, hist.as<uint32_t>(), g.nblocks);  // ids are a byte stream: 16 per load
        }
        QEH_HIP(hipGetLastError());
        QEH_TRY(exclusive_scan_u32(ctx, hist.as<uint32_t>(), offs.as<uint64_t>(), (int64_t)g.ndig * g.nblocks, nullptr));
        QEH_TRY(counts_from_hist(ctx, hist, g, n_parts, counts));
        for (int p = 0; p < n_parts; ++p) kept += counts[p];
    }
    int made = 0, s = QEH_OK;
    for (; made < n_move; ++made)
        if ((s = alloc_column(ctx, cols[move_idx[made]].dtype, kept, false, &out_cols[made])) != QEH_OK) break;
    if (s == QEH_OK && kept > 0) {
        const PmCols pc = pack_pm_cols(cols, move_idx, out_cols, nullptr, n_move);
        KernelTimer kt(ctx, "partition_move");
        const bool small = n_parts < kPsDig && !std::getenv("QEH_PM_GENERIC");  // ids 0..n_parts (the drop id)
        launch_part_scatter(ctx, n_move, small, rs_ballot(ctx), ids.as<uint8_t>(), n, g.seg, offs.as<uint64_t>(), g.nblocks,
                            pc, (uint32_t)n_parts);
        if (hipGetLastError() != hipSuccess) s = fail(QEH_E_HIP, "filter-partition move launch failed");
    }
    if (s == QEH_OK) {
        const hipError_t e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) s = fail(QEH_E_HIP, std::string("filter-partition move: ") + hipGetErrorString(e));
    }
    if (s != QEH_OK)
        for (int q = 0; q < made; ++q) qeh_column_release(ctx, &out_cols[q]);
    return s;
}

extern "C" int qeh_partition_range(qeh_ctx *ctx, const qeh_column *key, const int64_t *boundaries, int n_boundaries,
                                   int64_t *counts, qeh_column *out_perm) {
    if (!ctx || !key || !counts || !out_perm || n_boundaries < 0 || n_boundaries >= kRadix ||
        (n_boundaries > 0 && !boundaries))
        return fail(QEH_E_INVALID, "qeh_partition_range: bad argument (0..255 boundaries)");
    DeviceGuard dg(ctx->device);
    QEH_TRY(check_column(*key, "partition key"));
    if (is_temporal(key->dtype)) return fail(QEH_E_UNSUPPORTED, "temporal range partition keys are not supported on the device");
    const int64_t n = key->length;
    DevBuf bd;
    QEH_TRY(bd.alloc(ctx, (size_t)std::max(n_boundaries, 1) * 8));
    if (n_boundaries > 0)
        QEH_HIP(hipMemcpyAsync(bd.p, boundaries, (size_t)n_boundaries * 8, hipMemcpyHostToDevice, ctx->stream));
    QEH_HIP(hipStreamSynchronize(ctx->stream));
    const ColRef kc = make_colref(*key);
    const int is_i64 = key->dtype == QEH_DT_INT64;
    return partition_perm(
        ctx, n, n_boundaries + 1,
        [&](uint64_t *ids, uint32_t *idx) {
            hipLaunchKernelGGL(k_range_ids_first_below, dim3(grid_for(ctx, n, kBlock * 8, 8)), dim3(kBlock), 0, ctx->stream,
                               kc, n, bd.as<int64_t>(), n_boundaries, is_i64, ids, idx);
        },
        "range_partition", counts, out_perm);
}
