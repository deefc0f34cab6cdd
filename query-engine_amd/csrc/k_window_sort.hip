// Window functions over the sorted order (qeh_row_number, qeh_window): the general path, for every
// shape the partitioning path (k_window.hip, k_window3.hip) does not take.  The rows are sorted by
// (PARTITION BY keys, ORDER BY keys) with the radix sort of k_sort.hip; flags mark where a partition
// or a peer group starts, chunked max-scans turn them into each row's start, and one kernel writes
// the results into input order.
//
// Reference: the Window arm passes its input through (crates/query-executor/src/executor.rs:76-80),
// so the semantics are the intended ones of SURVEY.md §8.0: ROW_NUMBER numbers rows 1.. within each
// PARTITION BY group in ORDER BY order, ties by input position (docs/WINDOW_FUNCTIONS.md:44-65),
// output aligned to input order.
#include <algorithm>
#include <vector>

#include "../../include/qeh_plan.h"
#include "device_common.h"
#include "sort.h"

namespace qeh {

// ---- ROW_NUMBER ----------------------------------------------------------------------------
// flags[i] = 1 when sorted row i starts a new partition (partition columns differ from row i-1)
// One gather per row: each lane loads its row's keys through the permutation and takes the
// previous row's from the lane below (lane 0 loads its predecessor itself), halving the random
// reads of comparing perm[i-1] with perm[i] directly.  Whole workgroups step together, so every
// lane of a wave reaches the shuffles.
__global__ void k_part_flags(KeyCols part, const uint32_t *__restrict__ perm, int64_t n, uint32_t *__restrict__ flags) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = (int64_t)blockIdx.x * blockDim.x; base < n; base += stride) {
        const int64_t i = base + threadIdx.x;
        const bool act = i < n;
        const int64_t b = act ? (int64_t)perm[i] : 0;
        const bool own_prev = act && lane == 0 && i > 0;
        const int64_t a = own_prev ? (int64_t)perm[i - 1] : 0;
        uint32_t f = 0;
        for (int c = 0; c < part.n; ++c) {
            const int vb = act && col_valid(part.c[c], b) ? 1 : 0;
            const int64_t xb = vb ? load_i64(part.c[c], b) : 0;
            int va = __shfl_up(vb, 1, 64);
            int64_t xa = __shfl_up(xb, 1, 64);
            if (own_prev) {
                va = col_valid(part.c[c], a) ? 1 : 0;
                xa = va ? load_i64(part.c[c], a) : 0;
            }
            if (va != vb || (va && xa != xb)) f = 1;
        }
        if (act) flags[i] = i == 0 ? 1u : f;
    }
}

// single partition key: compare the sorted encodings (coalesced) instead of
// gathering the key column through the permutation.  shift >= the key width means the
// partition key occupies no bits (one distinct value): only row 0 starts a partition (a shift
// by the full width would be undefined and the hardware masks it to 0).
template <typename KeyT>
__global__ void k_part_flags_enc(const KeyT *__restrict__ enc, int64_t n, uint32_t *__restrict__ flags, int shift = 0) {
    const bool one_part = shift >= (int)(8 * sizeof(KeyT));
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        flags[i] = i == 0 || (!one_part && (enc[i] >> shift) != (enc[i - 1] >> shift));
}

// Row numbers without materialising partition ids: rn(i) = i - start(i) + 1,
// start(i) = the last partition start <= i.  Chunks of kRnChunk sorted
// positions: (1) each chunk's last start, (2) an exclusive prefix max over
// chunks, (3) per chunk a block max-scan seeded with (2), then the scatter
// rn[perm[i]] into input order.  No partition count is read back.
constexpr int kRnPer = 16;
constexpr int64_t kRnChunk = (int64_t)kBlock * kRnPer;

__global__ __launch_bounds__(kBlock) void k_rn_chunk_last(const uint32_t *__restrict__ flags, int64_t n, int64_t nchunks,
                                                          int64_t *__restrict__ last) {
    __shared__ int64_t red[kBlock / 64];
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        int64_t m = -1;
        const int64_t base = c * kRnChunk;
        for (int j = 0; j < kRnPer; ++j) {
            const int64_t i = base + (int64_t)j * kBlock + threadIdx.x;
            if (i < n && flags[i]) m = i > m ? i : m;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const int64_t o = __shfl_xor(m, d, 64);
            m = o > m ? o : m;
        }
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
        __syncthreads();
        if (threadIdx.x == 0) {
            for (int w = 1; w < kBlock / 64; ++w) m = red[w] > m ? red[w] : m;
            last[c] = m;
        }
        __syncthreads();
    }
}

// in place: last[c] <- max(last[0..c-1]) (exclusive), one workgroup
__global__ __launch_bounds__(1024) void k_rn_prefix_max(int64_t *__restrict__ last, int64_t nchunks) {
    __shared__ int64_t part[1024];
    const int t = threadIdx.x;
    const int64_t per = (nchunks + 1023) / 1024, lo = (int64_t)t * per, hi = lo + per < nchunks ? lo + per : nchunks;
    int64_t m = -1;
    for (int64_t c = lo; c < hi; ++c) m = last[c] > m ? last[c] : m;
    part[t] = m;
    __syncthreads();
    if (t == 0) {
        int64_t run = -1;
        for (int i = 0; i < 1024; ++i) {
            const int64_t x = part[i];
            part[i] = run;
            run = x > run ? x : run;
        }
    }
    __syncthreads();
    int64_t run = part[t];
    for (int64_t c = lo; c < hi; ++c) {
        const int64_t x = last[c];
        last[c] = run;
        run = x > run ? x : run;
    }
}

// PAIRS: instead of scattering rn[perm[i]] (1e9 random 8-byte writes), write the pairs
// (perm[i], rn) in sorted order; one stable radix pass on the destination's top bits then
// groups them by output window and k_rn_scatter_windows writes one window at a time
template <bool PAIRS>
__global__ __launch_bounds__(kBlock) void k_rn_write(const uint32_t *__restrict__ flags, const int64_t *__restrict__ carry,
                                                     const uint32_t *__restrict__ perm, int64_t n, int64_t nchunks,
                                                     int64_t *__restrict__ rn, uint32_t *__restrict__ pair_dst,
                                                     uint32_t *__restrict__ pair_rn) {
    __shared__ int64_t wmax[kBlock / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        // thread t owns kRnPer consecutive positions
        const int64_t base = c * kRnChunk + (int64_t)t * kRnPer;
        uint32_t f[kRnPer];
        int64_t m = -1;
#pragma unroll
        for (int j = 0; j < kRnPer; ++j) {
            const int64_t i = base + j;
            f[j] = i < n ? flags[i] : 0u;
            if (f[j]) m = i;
        }
        // exclusive max-scan of the threads' last starts, seeded with the chunks before
        int64_t incl = m;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t o = __shfl_up(incl, d, 64);
            if (lane >= d) incl = o > incl ? o : incl;
        }
        if (lane == 63) wmax[w] = incl;
        __syncthreads();
        int64_t start = carry[c];
        for (int q = 0; q < w; ++q) start = wmax[q] > start ? wmax[q] : start;
        const int64_t prev = __shfl_up(incl, 1, 64);
        if (lane > 0) start = prev > start ? prev : start;
#pragma unroll
        for (int j = 0; j < kRnPer; ++j) {
            const int64_t i = base + j;
            if (f[j]) start = i;
            if (i < n) {
                if (PAIRS) {
                    pair_dst[i] = perm[i];
                    pair_rn[i] = (uint32_t)(i - start + 1);
                } else {
                    rn[perm[i]] = i - start + 1;
                }
            }
        }
        __syncthreads();
    }
}

// pairs grouped by output window (destination >> shift): consecutive workgroups write inside
// one window at a time, so the partial-line writes meet in L2 / the Infinity Cache instead of HBM
__global__ void k_rn_scatter_windows(const uint32_t *__restrict__ dst, const uint32_t *__restrict__ val, int64_t n,
                                     int64_t *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        out[dst[i]] = (int64_t)val[i];
}

// start of every window in the window-grouped pairs (empty windows start where the next begins)
__global__ void k_rn_window_starts(const uint32_t *__restrict__ dst, int64_t n, int shift, int64_t nwin,
                                   int64_t *__restrict__ start) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t w = i < n ? (int64_t)(dst[i] >> shift) : nwin;
        const int64_t wp = i > 0 ? (int64_t)(dst[i - 1] >> shift) : -1;
        for (int64_t q = wp + 1; q <= w; ++q) start[q] = i;  // windows (wp, w] begin at i
    }
}

// XCD-local windows: workgroup b runs on XCD b % 8 (round-robin dispatch), and the workgroups of
// one XCD walk that XCD's windows (w = xcd, xcd + 8, ...) together, so a window's output lines
// (2 MB) are completed inside one L2 before they are written back
__global__ void k_rn_scatter_xcd(const uint32_t *__restrict__ dst, const uint32_t *__restrict__ val,
                                 const int64_t *__restrict__ start, int64_t nwin, int64_t *__restrict__ out) {
    constexpr int kXcd = 8;
    const int xcd = blockIdx.x % kXcd;
    const int64_t per = gridDim.x / kXcd, me = blockIdx.x / kXcd;
    for (int64_t w = xcd; w < nwin; w += kXcd) {
        const int64_t a = start[w], b = start[w + 1];
        for (int64_t i = a + me * blockDim.x + threadIdx.x; i < b; i += per * blockDim.x) out[dst[i]] = (int64_t)val[i];
    }
}

}  // namespace qeh

using namespace qeh;

// The sort keys of a window: the PARTITION BY keys (ascending), then the ORDER BY keys as given.
// Utf8 keys are replaced by their dictionary codes, which compare as the strings do, temporal keys
// by views of their physical integers.
struct WindowKeys {
    Utf8Keys pk, ok;                  // own the codes
    const qeh_column *part, *order;   // the keys to use: the caller's, or pk's / ok's
    std::vector<qeh_column> all;
    std::vector<int8_t> asc;
};

static int make_window_keys(qeh_ctx *ctx, const qeh_column *part_keys, int n_part, const qeh_column *order_keys, int n_order,
                            const int8_t *ascending, WindowKeys *w) {
    w->part = part_keys, w->order = order_keys;
    if (any_recoded_key(part_keys, n_part) || any_recoded_key(order_keys, n_order)) {
        QEH_TRY(encode_utf8_keys(ctx, part_keys, n_part, &w->pk));
        QEH_TRY(encode_utf8_keys(ctx, order_keys, n_order, &w->ok));
        w->part = w->pk.keys.data(), w->order = w->ok.keys.data();
    }
    for (int j = 0; j < n_part; ++j) w->all.push_back(w->part[j]), w->asc.push_back(1);
    for (int j = 0; j < n_order; ++j) w->all.push_back(w->order[j]), w->asc.push_back(ascending ? ascending[j] : 1);
    return QEH_OK;
}

// flags[i] = sorted row i starts a partition: from the sorted encodings when they determine the
// (single) partition key, else by comparing the key columns through the permutation.  have_sort:
// rs holds the sort that produced perm (false: OVER () or no keys, perm is the identity).
static void launch_part_flags(qeh_ctx *ctx, const RadixState &rs, const qeh_column *part_keys, int n_part, int n_order,
                              bool have_sort, const uint32_t *perm, int64_t n, uint32_t *flags) {
    KeyCols pk{};
    pk.n = n_part;
    for (int j = 0; j < n_part; ++j) pk.c[j] = make_colref(part_keys[j]);
    const int grid = grid_for(ctx, n, kBlock * 8, 8);
    const int sh = rs.part_shift >= 0 ? rs.part_shift : 0;
    const bool enc_ok = have_sort && n_part == 1 && (rs.enc_injective || (rs.part_shift >= 0 && n_order == 1));
    if (enc_ok && rs.key32)
        hipLaunchKernelGGL(k_part_flags_enc<uint32_t>, dim3(grid), dim3(kBlock), 0, ctx->stream, rs.k[rs.cur].as<uint32_t>(), n,
                           flags, sh);
    else if (enc_ok)
        hipLaunchKernelGGL(k_part_flags_enc<uint64_t>, dim3(grid), dim3(kBlock), 0, ctx->stream, rs.k[rs.cur].as<uint64_t>(), n,
                           flags, sh);
    else
        hipLaunchKernelGGL(k_part_flags, dim3(grid), dim3(kBlock), 0, ctx->stream, pk, perm, n, flags);
}

// carry[c] = the last flagged position before chunk c (-1: none)
static void launch_chunk_carry(qeh_ctx *ctx, const uint32_t *flags, int64_t n, int64_t nchunks, int64_t *carry) {
    hipLaunchKernelGGL(k_rn_chunk_last, dim3(gc_of(ctx, nchunks)), dim3(kBlock), 0, ctx->stream, flags, n, nchunks, carry);
    hipLaunchKernelGGL(k_rn_prefix_max, dim3(1), dim3(1024), 0, ctx->stream, carry, nchunks);
}

extern "C" int qeh_row_number(qeh_ctx *ctx, const qeh_column *part_keys, int n_part, const qeh_column *order_keys,
                              int n_order, const int8_t *ascending, qeh_column *out_rn) {
    if (!ctx || !out_rn || (n_part + n_order) < 1) return fail(QEH_E_INVALID, "qeh_row_number: bad argument");
    if (n_part > kMaxGroupKeys) return fail(QEH_E_UNSUPPORTED, "at most 4 PARTITION BY keys on the device");
    DeviceGuard dg(ctx->device);
    WindowKeys wk;
    QEH_TRY(make_window_keys(ctx, part_keys, n_part, order_keys, n_order, ascending, &wk));
    part_keys = wk.part, order_keys = wk.order;
    int64_t n;
    QEH_TRY(check_sort_keys(wk.all.data(), (int)wk.all.size(), &n));
    if (n_part >= 1 && n_order == 1) {  // bounded integer partition keys: partition instead of sorting
        const int s = window_msd_keys(ctx, QEH_WIN_ROW_NUMBER, part_keys, n_part, order_keys[0], wk.asc[n_part] != 0, 0, nullptr,
                                      nullptr, out_rn);
        if (s != kWindowMsdNotEligible) return s;
    }
    RadixState rs;
    QEH_TRY(sort_perm(ctx, wk.all.data(), (int)wk.all.size(), wk.asc.data(), n, rs));
    QEH_TRY(alloc_column(ctx, QEH_DT_INT64, n, false, out_rn));
    if (n == 0) return QEH_OK;
    const uint32_t *perm = rs.v[rs.cur].as<uint32_t>();
    auto bail = [&](int s) {
        qeh_column_release(ctx, out_rn);
        return s;
    };
    DevBuf flags, seg;
    int s = flags.alloc(ctx, (size_t)n * 4);
    if (s != QEH_OK) return bail(s);
    {
        KernelTimer kt(ctx, "row_number");
        launch_part_flags(ctx, rs, part_keys, n_part, n_order, true, perm, n, flags.as<uint32_t>());
    }
    const int64_t nchunks = (n + kRnChunk - 1) / kRnChunk;
    s = seg.alloc(ctx, (size_t)nchunks * 8);
    if (s != QEH_OK) return bail(s);
    {
        KernelTimer kt(ctx, "row_number");
        launch_chunk_carry(ctx, flags.as<uint32_t>(), n, nchunks, seg.as<int64_t>());
    }
    const int dbits = bit_length((uint64_t)(n - 1));
    // Direct scatter by default.  QEH_RN_WINDOWED (experiment, slower): group the (destination,
    // rn) pairs into 2 MB output windows with two radix passes and scatter window by window with
    // the workgroups of one XCD per window — 138 vs 104 ms for cfg 5 (the passes cost 23 ms and
    // the windowed scatter did not beat the direct one; with one pass and 32 MB windows: 61 vs
    // 40 ms for the row-number stage).
    if (dbits <= 22 || !std::getenv("QEH_RN_WINDOWED")) {
        KernelTimer kt(ctx, "row_number");
        hipLaunchKernelGGL(k_rn_write<false>, dim3(gc_of(ctx, nchunks)), dim3(kBlock), 0, ctx->stream, flags.as<uint32_t>(),
                           seg.as<int64_t>(), perm, n, nchunks, (int64_t *)out_rn->values, nullptr, nullptr);
    } else {
        // (destination, rn) pairs in sorted order into the spare radix buffers, one stable 8-bit
        // pass on the destination's top bits (windows of 2^(dbits-8) rows), windowed scatter
        const int o = 1 - rs.cur;
        {
            KernelTimer kt(ctx, "row_number");
            hipLaunchKernelGGL(k_rn_write<true>, dim3(gc_of(ctx, nchunks)), dim3(kBlock), 0, ctx->stream,
                               flags.as<uint32_t>(), seg.as<int64_t>(), perm, n, nchunks, nullptr, rs.k[o].as<uint32_t>(),
                               rs.v[o].as<uint32_t>());
        }
        rs.cur = o;
        rs.key32 = true;
        // 2 MB output windows (2^18 rows): two stable passes on destination bits [dbits-12, dbits)
        const int wshift = dbits - 12;
        s = radix_pass_at(ctx, rs, wshift);
        if (s == QEH_OK) s = radix_pass_at(ctx, rs, wshift + 8);
        DevBuf starts;
        const int64_t nwin = (int64_t)(((uint64_t)(n - 1) >> wshift) + 1);
        if (s == QEH_OK) s = starts.alloc(ctx, (size_t)(nwin + 1) * 8);
        if (s != QEH_OK) return bail(s);
        KernelTimer kt(ctx, "row_number");
        hipLaunchKernelGGL(k_rn_window_starts, dim3(grid_for(ctx, n + 1, kBlock * 8, 8)), dim3(kBlock), 0, ctx->stream,
                           rs.k[rs.cur].as<uint32_t>(), n, wshift, nwin, starts.as<int64_t>());
        const int gx = (int)std::max<int64_t>(8, ctx->props.multiProcessorCount * 4 / 8 * 8);
        hipLaunchKernelGGL(k_rn_scatter_xcd, dim3(gx), dim3(kBlock), 0, ctx->stream, rs.k[rs.cur].as<uint32_t>(),
                           rs.v[rs.cur].as<uint32_t>(), starts.as<int64_t>(), nwin, (int64_t *)out_rn->values);
    }
    QEH_HIP(hipGetLastError());
    QEH_HIP(hipStreamSynchronize(ctx->stream));
    return QEH_OK;
}

// ---- RANK / DENSE_RANK / NTILE / LAG / LEAD / FIRST_VALUE / LAST_VALUE -------------------
// Same sorted order as ROW_NUMBER.  In sorted positions: ps[i] = start of i's partition and
// qs[i] = start of its peer group (last flagged position <= i: the chunked max-scan of the row
// numbers), peer-group counts by an exclusive scan (DENSE_RANK), partition ends stored at their
// start (NTILE / LEAD / LAST_VALUE); one kernel then writes every row's result into input order.

// L[i] = last j <= i with flags[j] (k_rn_write's scan, writing the start instead of i - start + 1)
__global__ __launch_bounds__(kBlock) void k_seg_start(const uint32_t *__restrict__ flags, const int64_t *__restrict__ carry,
                                                      int64_t n, int64_t nchunks, int64_t *__restrict__ L) {
    __shared__ int64_t wmax[kBlock / 64];
    const int t = threadIdx.x, lane = t & 63, w = t >> 6;
    for (int64_t c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const int64_t base = c * kRnChunk + (int64_t)t * kRnPer;
        uint32_t f[kRnPer];
        int64_t m = -1;
#pragma unroll
        for (int j = 0; j < kRnPer; ++j) {
            const int64_t i = base + j;
            f[j] = i < n ? flags[i] : 0u;
            if (f[j]) m = i;
        }
        int64_t incl = m;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t o = __shfl_up(incl, d, 64);
            if (lane >= d) incl = o > incl ? o : incl;
        }
        if (lane == 63) wmax[w] = incl;
        __syncthreads();
        int64_t start = carry[c];
        for (int q = 0; q < w; ++q) start = wmax[q] > start ? wmax[q] : start;
        const int64_t prev = __shfl_up(incl, 1, 64);
        if (lane > 0) start = prev > start ? prev : start;
#pragma unroll
        for (int j = 0; j < kRnPer; ++j) {
            const int64_t i = base + j;
            if (f[j]) start = i;
            if (i < n) L[i] = start;
        }
        __syncthreads();
    }
}

__global__ void k_or_flags(uint32_t *__restrict__ a, const uint32_t *__restrict__ b, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        a[i] |= b[i];
}

// pend[ps[i]] = end of i's partition, written by its last row
__global__ void k_part_end(const uint32_t *__restrict__ fp, const int64_t *__restrict__ ps, int64_t n,
                           int64_t *__restrict__ pend) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        if (i == n - 1 || fp[i + 1]) pend[ps[i]] = i + 1;
}

__global__ void k_win_iota(uint32_t *__restrict__ p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
        p[i] = (uint32_t)i;
}

struct WinArgs {
    const uint32_t *perm;
    const int64_t *ps, *qs, *pend;
    const uint64_t *excl;  // exclusive scan of the peer flags
    const uint32_t *fq;    // peer flags
    ColRef arg;
    int64_t param;
    int64_t dflt;
    int has_dflt;
    int esz;               // argument element bytes (value functions)
};

template <int FUNC>
__global__ void k_window_out(WinArgs a, int64_t n, void *__restrict__ out, uint8_t *__restrict__ valid8) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = a.ps[i], row = a.perm[i];
        int64_t v = 0, src = -1;
        uint8_t ok = 1;
        if (FUNC == QEH_WIN_ROW_NUMBER) {
            v = i - s + 1;
        } else if (FUNC == QEH_WIN_RANK) {
            v = a.qs[i] - s + 1;
        } else if (FUNC == QEH_WIN_DENSE_RANK) {
            v = (int64_t)(a.excl[i] + a.fq[i] - a.excl[s]);
        } else if (FUNC == QEH_WIN_NTILE) {
            const int64_t size = a.pend[s] - s, r0 = i - s, q = size / a.param, r = size % a.param;
            v = r0 < r * (q + 1) ? r0 / (q + 1) + 1 : r + (r0 - r * (q + 1)) / q + 1;
        } else if (FUNC == QEH_WIN_LAG) {
            src = a.param <= i - s ? (int64_t)a.perm[i - a.param] : -2;
        } else if (FUNC == QEH_WIN_LEAD) {
            src = a.param < a.pend[s] - i ? (int64_t)a.perm[i + a.param] : -2;  // no i + param overflow
        } else if (FUNC == QEH_WIN_FIRST_VALUE) {
            src = a.perm[s];
        } else {  // LAST_VALUE: the partition's last row (whole-partition frame)
            src = a.perm[a.pend[s] - 1];
        }
        if (FUNC >= QEH_WIN_LAG) {
            if (src == -2) {
                ok = (uint8_t)a.has_dflt;
                v = a.dflt;
            } else {
                ok = col_valid(a.arg, src) ? 1 : 0;
                v = a.esz == 8 ? ((const int64_t *)a.arg.values)[src] : (int64_t)((const uint32_t *)a.arg.values)[src];
            }
            valid8[row] = ok;
            if (a.esz == 8) ((int64_t *)out)[row] = ok ? v : 0;
            else ((uint32_t *)out)[row] = ok ? (uint32_t)v : 0u;
        } else {
            ((int64_t *)out)[row] = v;
        }
    }
}

extern "C" int qeh_window(qeh_ctx *ctx, int32_t func, const qeh_column *part_keys, int n_part, const qeh_column *order_keys,
                          int n_order, const int8_t *ascending, const qeh_column *arg, int64_t param, const int64_t *dflt,
                          qeh_column *out) {
    if (!ctx || !out || n_part < 0 || n_order < 0) return fail(QEH_E_INVALID, "qeh_window: bad argument");
    if (func < QEH_WIN_ROW_NUMBER || func > QEH_WIN_LAST_VALUE) return fail(QEH_E_INVALID, "qeh_window: unknown function");
    if (n_part > kMaxGroupKeys || n_order > kMaxGroupKeys)
        return fail(QEH_E_UNSUPPORTED, "at most 4 PARTITION BY and 4 ORDER BY keys on the device");
    const bool value_fn = func >= QEH_WIN_LAG;
    if (func == QEH_WIN_NTILE && param < 1) return fail(QEH_E_INVALID, "NTILE needs a bucket count >= 1");
    if ((func == QEH_WIN_LAG || func == QEH_WIN_LEAD) && param < 0) return fail(QEH_E_INVALID, "LAG/LEAD offset must be >= 0");
    if (arg && is_temporal(arg->dtype)) {  // the values move as their physical integers and keep their dtype
        const qeh_column pa = physical_view(*arg);
        QEH_TRY(qeh_window(ctx, func, part_keys, n_part, order_keys, n_order, ascending, &pa, param, dflt, out));
        if (value_fn) out->dtype = arg->dtype;
        return QEH_OK;
    }
    int esz = 8;
    if (value_fn) {
        if (!arg) return fail(QEH_E_INVALID, "window value function needs an argument column");
        QEH_TRY(check_column(*arg, "window argument"));
        if (arg->dtype == QEH_DT_INT32 || arg->dtype == QEH_DT_FLOAT32) esz = 4;
        else if (arg->dtype != QEH_DT_INT64 && arg->dtype != QEH_DT_FLOAT64)
            return fail(QEH_E_UNSUPPORTED, "window value functions take Int32/Int64/Float32/Float64 on the device");
    }
    DeviceGuard dg(ctx->device);
    WindowKeys wk;  // (a Utf8 `arg` stays unsupported, above)
    QEH_TRY(make_window_keys(ctx, part_keys, n_part, order_keys, n_order, ascending, &wk));
    part_keys = wk.part, order_keys = wk.order;
    const bool have_keys = !wk.all.empty();
    int64_t n = arg ? arg->length : 0;  // OVER (): the argument column gives the row count
    if (have_keys) {
        QEH_TRY(check_sort_keys(wk.all.data(), (int)wk.all.size(), &n));
        if (value_fn && arg->length != n) return fail(QEH_E_INVALID, "window argument length mismatch");
    } else if (!arg) {
        return fail(QEH_E_INVALID, "qeh_window: OVER () needs a column for the row count");
    }
    if (func == QEH_WIN_ROW_NUMBER && have_keys)  // the dedicated path (pair-key sort, no peer state)
        return qeh_row_number(ctx, part_keys, n_part, order_keys, n_order, ascending, out);
    if (n_part >= 1 && n_order == 1) {  // bounded integer partition keys: partition instead of sorting
        const int s = window_msd_keys(ctx, func, part_keys, n_part, order_keys[0], wk.asc[n_part] != 0, param, arg, dflt, out);
        if (s != kWindowMsdNotEligible) return s;
    }
    const int odt = value_fn ? arg->dtype : QEH_DT_INT64;
    QEH_TRY(alloc_column(ctx, odt, n, value_fn, out));
    if (n == 0) return QEH_OK;
    auto bail = [&](int s) {
        qeh_column_release(ctx, out);
        return s;
    };
    RadixState rs;
    DevBuf iota;
    const uint32_t *perm;
    if (have_keys) {
        int s = sort_perm(ctx, wk.all.data(), (int)wk.all.size(), wk.asc.data(), n, rs);
        if (s != QEH_OK) return bail(s);
        perm = rs.v[rs.cur].as<uint32_t>();
    } else {
        if (iota.alloc(ctx, (size_t)n * 4) != QEH_OK) return bail(QEH_E_OOM);
        hipLaunchKernelGGL(k_win_iota, dim3(grid_for(ctx, n, kBlock * 8, 8)), dim3(kBlock), 0, ctx->stream, iota.as<uint32_t>(), n);
        perm = iota.as<uint32_t>();
    }
    const int grid = grid_for(ctx, n, kBlock * 8, 8);
    const int64_t nchunks = (n + kRnChunk - 1) / kRnChunk;
    DevBuf fp, fq, ps, qs, pend, excl, carry, valid8;
    if (fp.alloc(ctx, (size_t)n * 4) != QEH_OK || ps.alloc(ctx, (size_t)n * 8) != QEH_OK ||
        carry.alloc(ctx, (size_t)nchunks * 8) != QEH_OK)
        return bail(QEH_E_OOM);
    KernelTimer kt(ctx, "window");
    launch_part_flags(ctx, rs, part_keys, n_part, n_order, have_keys, perm, n, fp.as<uint32_t>());
    // L[i] = the last flagged position <= i
    auto seg_start = [&](const uint32_t *flags, int64_t *L) {
        launch_chunk_carry(ctx, flags, n, nchunks, carry.as<int64_t>());
        hipLaunchKernelGGL(k_seg_start, dim3(gc_of(ctx, nchunks)), dim3(kBlock), 0, ctx->stream, flags, carry.as<int64_t>(), n,
                           nchunks, L);
    };
    seg_start(fp.as<uint32_t>(), ps.as<int64_t>());
    WinArgs a{};
    a.perm = perm;
    a.ps = ps.as<int64_t>();
    a.param = param;
    a.esz = esz;
    if (func == QEH_WIN_RANK || func == QEH_WIN_DENSE_RANK) {
        // peer flags: partition start or any ORDER BY key changes
        if (fq.alloc(ctx, (size_t)n * 4) != QEH_OK) return bail(QEH_E_OOM);
        KeyCols ok{};
        ok.n = n_order;
        for (int j = 0; j < n_order; ++j) ok.c[j] = make_colref(order_keys[j]);
        if (n_order > 0) {
            hipLaunchKernelGGL(k_part_flags, dim3(grid), dim3(kBlock), 0, ctx->stream, ok, perm, n, fq.as<uint32_t>());
            hipLaunchKernelGGL(k_or_flags, dim3(grid), dim3(kBlock), 0, ctx->stream, fq.as<uint32_t>(), fp.as<uint32_t>(), n);
        } else if (hipMemcpyAsync(fq.p, fp.p, (size_t)n * 4, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) {
            return bail(fail(QEH_E_HIP, "qeh_window: device copy failed"));
        }
        a.fq = fq.as<uint32_t>();
        if (func == QEH_WIN_RANK) {
            if (qs.alloc(ctx, (size_t)n * 8) != QEH_OK) return bail(QEH_E_OOM);
            seg_start(fq.as<uint32_t>(), qs.as<int64_t>());
            a.qs = qs.as<int64_t>();
        } else {
            if (excl.alloc(ctx, (size_t)n * 8) != QEH_OK) return bail(QEH_E_OOM);
            int s = exclusive_scan_u32(ctx, fq.as<uint32_t>(), excl.as<uint64_t>(), n, nullptr);
            if (s != QEH_OK) return bail(s);
            a.excl = excl.as<uint64_t>();
        }
    }
    if (func == QEH_WIN_NTILE || func == QEH_WIN_LEAD || func == QEH_WIN_LAST_VALUE) {
        if (pend.alloc(ctx, (size_t)n * 8) != QEH_OK) return bail(QEH_E_OOM);
        hipLaunchKernelGGL(k_part_end, dim3(grid), dim3(kBlock), 0, ctx->stream, fp.as<uint32_t>(), ps.as<int64_t>(), n,
                           pend.as<int64_t>());
        a.pend = pend.as<int64_t>();
    }
    if (value_fn) {
        if (valid8.alloc(ctx, (size_t)n) != QEH_OK) return bail(QEH_E_OOM);
        a.arg = make_colref(*arg);
        a.has_dflt = dflt != nullptr;
        if (dflt) a.dflt = esz == 8 ? *dflt : (int64_t)(uint32_t)*dflt;
    }
#define QEH_WIN(F)                                                                                                        \
    hipLaunchKernelGGL(k_window_out<F>, dim3(grid), dim3(kBlock), 0, ctx->stream, a, n, out->values, valid8.as<uint8_t>())
    switch (func) {
        case QEH_WIN_ROW_NUMBER: QEH_WIN(QEH_WIN_ROW_NUMBER); break;  // OVER (): input order
        case QEH_WIN_RANK: QEH_WIN(QEH_WIN_RANK); break;
        case QEH_WIN_DENSE_RANK: QEH_WIN(QEH_WIN_DENSE_RANK); break;
        case QEH_WIN_NTILE: QEH_WIN(QEH_WIN_NTILE); break;
        case QEH_WIN_LAG: QEH_WIN(QEH_WIN_LAG); break;
        case QEH_WIN_LEAD: QEH_WIN(QEH_WIN_LEAD); break;
        case QEH_WIN_FIRST_VALUE: QEH_WIN(QEH_WIN_FIRST_VALUE); break;
        default: QEH_WIN(QEH_WIN_LAST_VALUE); break;
    }
#undef QEH_WIN
    if (hipGetLastError() != hipSuccess) return bail(fail(QEH_E_HIP, "qeh_window: kernel launch failed"));
    if (value_fn) {
        int s = qeh_bytes_to_validity(ctx, valid8.as<uint8_t>(), n, out->validity);
        if (s != QEH_OK) return bail(s);
        out->null_count = -1;
    }
    if (hipStreamSynchronize(ctx->stream) != hipSuccess) return bail(fail(QEH_E_HIP, "qeh_window: stream synchronize failed"));
    return QEH_OK;
}
