// The LDS-slice materialising INNER join (k_slice_count, k_slice_join_inplace, k_slice_join_b,
// k_slice_join_tail) over phase A of the slice pipeline (k_aggregate.hip).  Exports
// slice_join_materialise (aggregate.h).
#include <algorithm>
#include <cstdlib>

#include "aggregate.h"

namespace qeh {

// ---- LDS-slice materialising INNER join (BASELINE config 3) -----------------------------
// Same phase A as the aggregate (k_slice_partition: items = 16-bit key offset +
// the probe payload).  Phase B writes the joined rows: the build payload is
// stored in the u16 table as (a - amin) + 1, so a slice in LDS answers both
// "matches?" and "with which value?".  Rows leave in slice order (the join's
// row order is not part of its contract); each wave reserves
// its matches with one atomic per 512 items and writes them contiguously.
// write the wave's matches of one 8-items-per-lane step at out[*base ...]
// (j-major, lanes in order within j: contiguous stores), advancing *base
__device__ __forceinline__ void emit_matches(const uint32_t *e, const int64_t *v, const bool *live, int64_t amin,
                                             uint64_t *base, int64_t *__restrict__ out_v, int64_t *__restrict__ out_a) {
    uint64_t b = *base;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const bool m = live[j] && e[j] != 0u;
        const uint64_t mask = __ballot(m);
        if (m) {
            const uint64_t pos = b + mbcnt(mask);
            out_v[pos] = v[j];
            out_a[pos] = (int64_t)(e[j] - 1u) + amin;
        }
        b += popc64(mask);
    }
    *base = b;
}

__device__ __forceinline__ void load_slice(uint16_t *tslice, const HashTable &t, int b, int tid) {
    const uint64_t k0 = (uint64_t)b << kSliceBits;
    const uint64_t nk = t.range - k0 < (uint64_t)kSliceKeys ? t.range - k0 : (uint64_t)kSliceKeys;
    for (int i = tid * 8; i < kSliceKeys; i += kSliceBlock * 8) {
        v4u32 w = {0u, 0u, 0u, 0u};
        if ((uint64_t)i + 8 <= nk) {
            w = *(const v4u32 *)(t.payload16 + k0 + i);
        } else {
            for (int q = 0; q < 8; ++q)
                if ((uint64_t)(i + q) < nk) w[q >> 1] |= (uint32_t)t.payload16[k0 + i + q] << ((q & 1) * 16);
        }
        *(v4u32 *)&tslice[i] = w;
    }
}

// Phase B of the join in two passes, no atomics: EMIT = false counts each
// region's matches (keys only) into counts[slot]; after an exclusive scan of
// those (slot order), EMIT = true writes each region's matches from its base.
template <bool EMIT>
__global__ __launch_bounds__(kSliceBlock) void k_slice_join_b(SliceRegions rg, int nreg, HashTable t, int64_t amin,
                                                              uint32_t *__restrict__ counts, const uint64_t *__restrict__ bases,
                                                              int64_t *__restrict__ out_v, int64_t *__restrict__ out_a) {
    __shared__ __attribute__((aligned(16))) uint16_t tslice[kSliceKeys];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int W = kSliceBlock / 64;
    const int F = rg.F;
    const int64_t T = (int64_t)F * nreg;
    const int64_t s0 = (int64_t)blockIdx.x * T / gridDim.x, s1 = (int64_t)(blockIdx.x + 1) * T / gridDim.x;
    for (int64_t sb = s0; sb < s1;) {
        const int b = (int)(sb / nreg);
        const int64_t se = std::min<int64_t>(s1, (int64_t)(b + 1) * nreg);
        __syncthreads();
        load_slice(tslice, t, b, tid);
        __syncthreads();
        for (int64_t s = sb + wave; s < se; s += W) {
            const uint64_t reg = (uint64_t)(s - (int64_t)b * nreg) * F + b;
            const uint32_t n_r = rg.count[reg];
            const uint64_t rb = rg.rbase ? rg.rbase[s] : reg * rg.cap;
            const uint16_t *kp = rg.key + rb;
            const int64_t *vp = rg.val + rb;
            uint64_t base = EMIT ? bases[s] : 0;
            uint32_t matches = 0;
            for (uint32_t i0 = 0; i0 < n_r; i0 += 64 * 8) {
                uint32_t e[8];
                int64_t v[8];
                bool live[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const uint32_t i = i0 + j * 64 + lane;
                    live[j] = i < n_r;
                    const uint32_t ii = live[j] ? i : 0u;
                    e[j] = __builtin_nontemporal_load(kp + ii);
                    v[j] = EMIT ? __builtin_nontemporal_load(vp + ii) : 0;
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) e[j] = live[j] ? (uint32_t)tslice[e[j]] : 0u;
                if (EMIT) {
                    emit_matches(e, v, live, amin, &base, out_v, out_a);
                } else {
#pragma unroll
                    for (int j = 0; j < 8; ++j) matches += (uint32_t)popc64(__ballot(live[j] && e[j] != 0u));
                }
            }
            if (!EMIT && lane == 0) counts[s] = matches;
        }
        sb = se;
    }
}

// Exact region sizes for phase A of the materialising join: the same tile ->
// workgroup assignment as k_slice_partition, keys only (16-B loads), per-wave
// LDS counters; counts[b * grid + wg] (slice-major slots).
__global__ __launch_bounds__(kSliceBlock) void k_slice_count(const int64_t *__restrict__ key, int64_t kmin, uint64_t range,
                                                             int64_t n_tiles, int F, uint32_t *__restrict__ counts) {
    constexpr int W = kSliceBlock / 64;
    __shared__ uint32_t cnt[W][kSliceMaxF];
    const int tid = threadIdx.x, wave = tid >> 6;
    for (int i = tid; i < W * kSliceMaxF; i += kSliceBlock) (&cnt[0][0])[i] = 0;
    __syncthreads();
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t base = tile * kSliceTile;
        v2i64 kk[kSliceTile / (2 * kSliceBlock)];
#pragma unroll
        for (int q = 0; q < kSliceTile / (2 * kSliceBlock); ++q)
            kk[q] = __builtin_nontemporal_load((const v2i64 *)(key + base + 2 * ((int64_t)q * kSliceBlock + tid)));
#pragma unroll
        for (int q = 0; q < kSliceTile / (2 * kSliceBlock); ++q)
#pragma unroll
            for (int x = 0; x < 2; ++x) {
                const uint64_t o = (uint64_t)kk[q][x] - (uint64_t)kmin;
                if (o < range) atomicAdd(&cnt[wave][(uint32_t)(o >> kSliceBits)], 1u);
            }
    }
    __syncthreads();
    for (int b = tid; b < F; b += kSliceBlock) {
        uint32_t c = 0;
#pragma unroll
        for (int w = 0; w < W; ++w) c += cnt[w][b];
        counts[(uint64_t)b * gridDim.x + blockIdx.x] = c;
    }
}

// Phase B of the exact-layout join: the probe payload already sits at its
// output position (phase A wrote it into the output column), so each item only
// needs the build payload written beside it: read the 16-bit key offset, look
// it up in the LDS slice, store a.  Items without a match are counted (a
// non-zero count sends the host to the compacting two-pass emit).
__global__ __launch_bounds__(kSliceBlock) void k_slice_join_inplace(SliceRegions rg, int nreg, HashTable t, int64_t amin,
                                                                    int64_t *__restrict__ out_a,
                                                                    unsigned long long *__restrict__ misses) {
    __shared__ __attribute__((aligned(16))) uint16_t tslice[kSliceKeys];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int W = kSliceBlock / 64;
    const int F = rg.F;
    const int64_t T = (int64_t)F * nreg;
    const int64_t s0 = (int64_t)blockIdx.x * T / gridDim.x, s1 = (int64_t)(blockIdx.x + 1) * T / gridDim.x;
    uint32_t miss = 0;
    for (int64_t sb = s0; sb < s1;) {
        const int b = (int)(sb / nreg);
        const int64_t se = std::min<int64_t>(s1, (int64_t)(b + 1) * nreg);
        __syncthreads();
        load_slice(tslice, t, b, tid);
        __syncthreads();
        for (int64_t s = sb + wave; s < se; s += W) {
            const uint64_t reg = (uint64_t)(s - (int64_t)b * nreg) * F + b;
            const uint32_t n_r = rg.count[reg];
            const uint64_t rb = rg.rbase[s];
            const uint16_t *kp = rg.key + rb;
            int64_t *ap = out_a + rb;
            // the next 1024 keys are loaded before this batch's lookups and stores
            uint32_t e[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const uint32_t i = j * 64 + lane;
                e[j] = __builtin_nontemporal_load(kp + (i < n_r ? i : 0u));
            }
            for (uint32_t i0 = 0; i0 < n_r; i0 += 64 * 16) {
                uint32_t en[16];
                const uint32_t i1 = i0 + 64 * 16;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const uint32_t i = i1 + j * 64 + lane;
                    en[j] = __builtin_nontemporal_load(kp + (i < n_r ? i : 0u));
                }
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const uint32_t i = i0 + j * 64 + lane;
                    if (i < n_r) {
                        const uint32_t x = tslice[e[j]];
                        miss += x == 0u;
                        __builtin_nontemporal_store((int64_t)(x - 1u) + amin, ap + i);
                    }
                }
#pragma unroll
                for (int j = 0; j < 16; ++j) e[j] = en[j];
            }
        }
        sb = se;
    }
    const uint64_t m = wave_sum_u64(miss);
    if (lane == 0 && m) atomicAdd(misses, (unsigned long long)m);
}

// ragged tail (< one 8192-row tile): probe the u16 table directly and append
// after the regions' rows (a few waves: one atomic each per 512 rows)
__global__ __launch_bounds__(kBlock) void k_slice_join_tail(const int64_t *__restrict__ key, const int64_t *__restrict__ val,
                                                            int64_t n, HashTable t, int64_t amin, int64_t *__restrict__ out_v,
                                                            int64_t *__restrict__ out_a, unsigned long long *counter) {
    const int lane = threadIdx.x & 63;
    for (int64_t i0 = (int64_t)blockIdx.x * blockDim.x * 8 + (threadIdx.x & ~63) * 8; i0 < n;
         i0 += (int64_t)gridDim.x * blockDim.x * 8) {
        uint32_t e[8];
        int64_t v[8];
        bool live[8];
        uint32_t total = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int64_t i = i0 + j * 64 + lane;
            live[j] = i < n;
            e[j] = 0u;
            v[j] = 0;
            if (live[j]) {
                const uint64_t o = (uint64_t)key[i] - (uint64_t)t.kmin;
                if (o < t.range) e[j] = t.payload16[o];
                v[j] = val[i];
            }
            total += (uint32_t)popc64(__ballot(live[j] && e[j] != 0u));
        }
        unsigned long long b = 0;
        if (lane == 0 && total) b = atomicAdd(counter, (unsigned long long)total);
        uint64_t base = __shfl(b, 0, 64);
        emit_matches(e, v, live, amin, &base, out_v, out_a);
    }
}

int slice_join_materialise(qeh_ctx *ctx, const qeh_column &probe_key, const qeh_column &probe_val,
                           const qeh_column &build_key, const qeh_column &build_val, qeh_column *out_probe,
                           qeh_column *out_build, int64_t *out_rows) {
    if (std::getenv("QEH_NO_SLICES")) return kSliceJoinNotEligible;
    const ColRef pk = make_colref(probe_key), pv = make_colref(probe_val);
    if (probe_key.dtype != QEH_DT_INT64 || !fast_col_ok(pk) || !fast_col_ok(pv)) return kSliceJoinNotEligible;
    if (build_val.dtype != QEH_DT_INT64 || (build_val.validity && build_val.null_count != 0)) return kSliceJoinNotEligible;
    if (build_key.validity && build_key.null_count != 0) return kSliceJoinNotEligible;
    const int64_t n = probe_key.length;
    const int64_t n_tiles = n / kSliceTile;
    if (n_tiles == 0 || build_key.length == 0) return kSliceJoinNotEligible;
    // build payload as a frame-of-reference u16: (a - amin) + 1 in the direct table
    int64_t amin, amax, avalid;
    QEH_TRY(column_minmax(ctx, build_val, &amin, &amax, &avalid));
    if ((uint64_t)amax - (uint64_t)amin >= 0xFFFEull) return kSliceJoinNotEligible;
    BuiltTable bt;
    RowPayload rp;
    rp.values = (const int64_t *)build_val.values + build_val.offset;
    rp.bias = amin;
    QEH_TRY(build_join_table(ctx, build_key, rp, (uint64_t)amax - (uint64_t)amin, &bt));
    const HashTable &t = bt.t;
    if (!t.unique || t.kind != TK_DIRECT || !t.payload16) return kSliceJoinNotEligible;
    const uint64_t F = (t.range + kSliceKeys - 1) >> kSliceBits;
    if (F == 0 || F > (uint64_t)kSliceMaxF) return kSliceJoinNotEligible;
    if (table_bytes(t) < slice_min_bytes()) return kSliceJoinNotEligible;

    // Exact region layout: a key-only count pass sizes every (workgroup, slice) region, so
    // phase A writes the probe payload straight into the output column (slice-major, no
    // gaps) and phase B only adds the build payload beside it.  When some probe rows have
    // no match, the two-pass emit compacts the regions into fresh columns instead.
    const int grid = (int)std::min<int64_t>(ctx->props.multiProcessorCount, n_tiles);
    const uint64_t nreg = (uint64_t)grid * F;
    const uint64_t T = nreg;  // region slots, slice-major
    DevBuf kbuf, cbuf, counts, bases;
    QEH_TRY(cbuf.alloc(ctx, nreg * 4 + 64));
    QEH_TRY(counts.alloc(ctx, T * 4 + 16));
    QEH_TRY(bases.alloc(ctx, T * 8 + 16));
    FastIn in{};
    in.key = (const int64_t *)pk.values;
    in.acol[0] = (const int64_t *)pv.values;
    in.agg_colslot[0] = 0;
    uint64_t region_rows = 0;
    {
        KernelTimer kt(ctx, "join_probe");
        hipLaunchKernelGGL(k_slice_count, dim3(grid), dim3(kSliceBlock), 0, ctx->stream, in.key, t.kmin, t.range, n_tiles,
                           (int)F, counts.as<uint32_t>());
        QEH_HIP(hipGetLastError());
    }
    QEH_TRY(exclusive_scan_u32(ctx, counts.as<uint32_t>(), bases.as<uint64_t>(), (int64_t)T, &region_rows));
    QEH_TRY(kbuf.alloc(ctx, region_rows * 2 + 64));
    SliceRegions rg{};
    rg.key = kbuf.as<uint16_t>();
    rg.count = cbuf.as<uint32_t>();
    rg.overflow = rg.count + nreg;                                                                     // 4 B
    unsigned long long *counter = (unsigned long long *)(cbuf.as<char>() + ((nreg * 4 + 15) & ~15ull));  // 8 B
    unsigned long long *misses = counter + 1;                                                          // 8 B
    rg.cap = 1ull << 62;  // exact regions never overflow
    rg.F = (int32_t)F;
    rg.rbase = bases.as<uint64_t>();
    QEH_HIP(hipMemsetAsync(rg.overflow, 0, 4, ctx->stream));
    QEH_HIP(hipMemsetAsync(counter, 0, 16, ctx->stream));
    QEH_TRY(alloc_column(ctx, probe_val.dtype, n, false, out_probe));
    int st = alloc_column(ctx, QEH_DT_INT64, n, false, out_build);
    if (st != QEH_OK) {
        qeh_column_release(ctx, out_probe);
        return st;
    }
    rg.val = (int64_t *)out_probe->values;
    int64_t *oa = (int64_t *)out_build->values;
    const int gridB = ctx->props.multiProcessorCount;
    {
        KernelTimer kt(ctx, "join_probe");
        // phase A with no predicate and one payload column, under this timer
        launch_slice_partition(ctx, in, PredPlan{}, 0, 1, t.kmin, t.range, n_tiles, grid, rg, ctx->stream, nullptr, nullptr,
                               nullptr);
        hipLaunchKernelGGL(k_slice_join_inplace, dim3(gridB), dim3(kSliceBlock), 0, ctx->stream, rg, grid, t, amin, oa,
                           misses);
        if (hipGetLastError() != hipSuccess) st = fail(QEH_E_HIP, "slice join launch failed");
    }
    uint64_t nmiss = 0;
    if (st == QEH_OK) st = read_small(ctx, &nmiss, misses, 8);
    qeh_column cv = *out_probe, ca = *out_build;  // the columns the tail appends to
    if (st == QEH_OK && nmiss != 0) {
        // some probe rows have no match: compact the regions (read from the first output
        // column) into fresh columns with the two-pass emit
        qeh_column cv2{}, ca2{};
        DevBuf counts2, bases2;
        st = alloc_column(ctx, probe_val.dtype, n, false, &cv2);
        if (st == QEH_OK) st = alloc_column(ctx, QEH_DT_INT64, n, false, &ca2);
        if (st == QEH_OK) st = counts2.alloc(ctx, T * 4 + 16);
        if (st == QEH_OK) st = bases2.alloc(ctx, T * 8 + 16);
        if (st == QEH_OK) {
            KernelTimer kt(ctx, "join_probe");
            hipLaunchKernelGGL((k_slice_join_b<false>), dim3(gridB), dim3(kSliceBlock), 0, ctx->stream, rg, grid, t, amin,
                               counts2.as<uint32_t>(), nullptr, nullptr, nullptr);
        }
        if (st == QEH_OK) st = exclusive_scan_u32(ctx, counts2.as<uint32_t>(), bases2.as<uint64_t>(), (int64_t)T, &region_rows);
        if (st == QEH_OK) {
            KernelTimer kt(ctx, "join_probe");
            hipLaunchKernelGGL((k_slice_join_b<true>), dim3(gridB), dim3(kSliceBlock), 0, ctx->stream, rg, grid, t, amin,
                               nullptr, bases2.as<uint64_t>(), (int64_t *)cv2.values, (int64_t *)ca2.values);
            if (hipGetLastError() != hipSuccess) st = fail(QEH_E_HIP, "slice join launch failed");
        }
        if (st == QEH_OK && hipStreamSynchronize(ctx->stream) != hipSuccess) st = fail(QEH_E_HIP, "slice join sync failed");
        if (st == QEH_OK) {
            qeh_column_release(ctx, out_probe);
            qeh_column_release(ctx, out_build);
            *out_probe = cv = cv2;
            *out_build = ca = ca2;
        } else {
            if (cv2.values) qeh_column_release(ctx, &cv2);
            if (ca2.values) qeh_column_release(ctx, &ca2);
        }
    }
    if (st == QEH_OK) {
        KernelTimer kt(ctx, "join_probe");
        const int64_t done = n_tiles * kSliceTile;
        fill_i64(ctx, 1, 1, (int64_t *)counter, 1, (int64_t)region_rows);
        if (done < n)
            hipLaunchKernelGGL(k_slice_join_tail, dim3(grid_for(ctx, n - done, kBlock * 8, 2)), dim3(kBlock), 0, ctx->stream,
                               in.key + done, in.acol[0] + done, n - done, t, amin, (int64_t *)cv.values,
                               (int64_t *)ca.values, counter);
        if (hipGetLastError() != hipSuccess) st = fail(QEH_E_HIP, "slice join launch failed");
    }
    uint64_t rows = 0;
    if (st == QEH_OK) st = read_small(ctx, &rows, counter, 8);
    if (st != QEH_OK) {
        qeh_column_release(ctx, out_probe);
        qeh_column_release(ctx, out_build);
        return st;
    }
    out_probe->length = (int64_t)rows;
    out_build->length = (int64_t)rows;
    *out_rows = (int64_t)rows;
    return QEH_OK;
}

}  // namespace qeh
