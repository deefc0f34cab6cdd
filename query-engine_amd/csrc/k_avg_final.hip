// AVG's last step on the device: out = (double)sum / (double)count, NULL where count is NULL or <= 0.
//
// evaluate_aggregate (crates/query-executor/src/operators.rs:770-808) computes AVG over one array as
// compute::sum(arr).unwrap_or(0) as f64 / count, None when count == 0.  A partial/final plan
// (crates/query-distributed/src/planner.rs:200-226) cannot merge AVG states, so the distributed layer
// carries SUM and COUNT partials, merges each with its own final aggregate and divides here.
//
// Int32 inputs: arrow's compute::sum over an Int32Array wraps in 32 bits, and the Int64 sum of
// 32-bit-wrapped partials is congruent to the job-wide sum mod 2^32, so wrapping the merged sum to
// 32 bits once and sign-extending gives the reference's (double)(int32_t) sum, overflow included.
//
// One streaming pass: a wave takes 64 rows at a time (kAvgRows such runs per iteration, so several
// loads are in flight), lane 0 writes the run's 64-bit validity word from a ballot, and the NULLs are
// counted from the same ballots: every workgroup stores its count to its own slot and the host adds
// the slots up (with one atomic per wave on one shared word a 2^20-row call took 56 us instead of 8).
#include "device_common.h"
#include "ops.h"

namespace qeh {

constexpr int kAvgRows = 4;

template <bool kSumF64, bool kWrap32>
__global__ __launch_bounds__(kBlock) void k_avg_finalize(const void *__restrict__ sum, const uint8_t *__restrict__ sum_valid,
                                                         int64_t sum_bit0, const int64_t *__restrict__ cnt,
                                                         const uint8_t *__restrict__ cnt_valid, int64_t cnt_bit0, int64_t n,
                                                         double *__restrict__ out, uint64_t *__restrict__ out_valid,
                                                         uint64_t *__restrict__ block_nulls) {
    const int lane = threadIdx.x & 63;
    const int64_t nchunks = (n + 64 * kAvgRows - 1) / (64 * kAvgRows);
    const int64_t wstride = (int64_t)gridDim.x * (blockDim.x / 64);
    uint64_t wave_nulls = 0;  // (kept by lane 0)
    for (int64_t w = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); w < nchunks; w += wstride) {
        const int64_t base = w * 64 * kAvgRows;
        // every load of the iteration is issued before the first result is needed: the values are read
        // whatever the bitmaps say (rows below n are always readable) and masked afterwards
        int64_t c[kAvgRows], sb[kAvgRows];
        bool cok[kAvgRows], sok[kAvgRows];
#pragma unroll
        for (int r = 0; r < kAvgRows; ++r) {
            const int64_t row = base + r * 64 + lane;
            const bool live = row < n;
            c[r] = live ? cnt[row] : 0;
            sb[r] = live ? ((const int64_t *)sum)[row] : 0;
            cok[r] = live && (cnt_valid == nullptr || bit_at(cnt_valid, cnt_bit0 + row));
            sok[r] = live && (sum_valid == nullptr || bit_at(sum_valid, sum_bit0 + row));
        }
#pragma unroll
        for (int r = 0; r < kAvgRows; ++r) {
            const int64_t row0 = base + r * 64;
            if (row0 >= n) break;  // wave-uniform
            const int64_t row = row0 + lane;
            // a NULL sum reads as 0 (the reference's unwrap_or(0)); whether the row is NULL is the count's call
            double s = 0.0;
            if (sok[r]) s = kSumF64 ? as_f64(sb[r]) : kWrap32 ? (double)(int32_t)(uint32_t)sb[r] : (double)sb[r];
            const bool valid = cok[r] && c[r] > 0;
            if (row < n) out[row] = valid ? s / (double)c[r] : 0.0;
            const uint64_t vb = __ballot(valid);
            if (lane == 0) {
                out_valid[row0 >> 6] = vb;
                const int64_t rows = n - row0 < 64 ? n - row0 : 64;
                wave_nulls += (uint64_t)rows - popc64(vb);
            }
        }
    }
    __shared__ uint64_t wn[kBlock / 64];
    if (lane == 0) wn[threadIdx.x >> 6] = wave_nulls;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t b = 0;
#pragma unroll
        for (int i = 0; i < kBlock / 64; ++i) b += wn[i];
        block_nulls[blockIdx.x] = b;  // every workgroup writes its slot: nothing to zero
    }
}

}  // namespace qeh

using namespace qeh;

extern "C" int qeh_avg_finalize(qeh_ctx *ctx, const qeh_column *sum, const qeh_column *count, int32_t input_dtype,
                                qeh_column *out) {
    if (!ctx || !sum || !count || !out) return fail(QEH_E_INVALID, "qeh_avg_finalize: bad argument");
    const bool in_int = input_dtype == QEH_DT_INT32 || input_dtype == QEH_DT_INT64;
    const bool in_float = input_dtype == QEH_DT_FLOAT32 || input_dtype == QEH_DT_FLOAT64;
    if (!in_int && !in_float) return fail(QEH_E_TYPE, "Unsupported type for AVG");
    // SUM's result type for that input (operators.rs:751-768): Int64 for integers, Float64 for floats
    if (sum->dtype != (in_int ? QEH_DT_INT64 : QEH_DT_FLOAT64))
        return fail(QEH_E_TYPE, "qeh_avg_finalize: sum must be Int64 for integer inputs, Float64 for float inputs");
    if (count->dtype != QEH_DT_INT64) return fail(QEH_E_TYPE, "qeh_avg_finalize: count must be Int64");
    if (sum->length != count->length || sum->length < 0 || sum->offset < 0 || count->offset < 0)
        return fail(QEH_E_INVALID, "qeh_avg_finalize: sum and count lengths differ");
    const int64_t n = sum->length;
    if (n > 0 && (!sum->values || !count->values)) return fail(QEH_E_INVALID, "qeh_avg_finalize: null values buffer");
    DeviceGuard dg(ctx->device);
    QEH_TRY(alloc_column(ctx, QEH_DT_FLOAT64, n, true, out));
    out->null_count = 0;
    if (n == 0) return QEH_OK;
    const void *sv = (const char *)sum->values + sum->offset * 8;
    const int64_t *cv = (const int64_t *)count->values + count->offset;
    const uint8_t *sm = (const uint8_t *)sum->validity, *cm = (const uint8_t *)count->validity;
    const int grid = grid_for(ctx, n, kBlock * kAvgRows, 8);
    void *scr = nullptr;
    int s = scratch_zeroed(ctx, (size_t)grid * 8, &scr);
    if (s != QEH_OK) {
        qeh_column_release(ctx, out);
        return s;
    }
    {
        KernelTimer kt(ctx, "avg_finalize");
#define QEH_AVG(F64, WRAP)                                                                                              \
    hipLaunchKernelGGL((k_avg_finalize<F64, WRAP>), dim3(grid), dim3(kBlock), 0, ctx->stream, sv, sm, sum->offset, cv, cm, \
                       count->offset, n, (double *)out->values, (uint64_t *)out->validity, (uint64_t *)scr)
        if (in_float) QEH_AVG(true, false);
        else if (input_dtype == QEH_DT_INT32) QEH_AVG(false, true);
        else QEH_AVG(false, false);
#undef QEH_AVG
    }
    hipError_t e = hipGetLastError();
    std::vector<uint64_t> per_block(grid);
    s = e == hipSuccess ? read_small(ctx, per_block.data(), scr, (size_t)grid * 8) : fail(QEH_E_HIP, std::string("k_avg_finalize: ") + hipGetErrorString(e));
    if (s != QEH_OK) {
        qeh_column_release(ctx, out);
        return s;
    }
    out->null_count = 0;
    for (uint64_t b : per_block) out->null_count += (int64_t)b;
    return QEH_OK;
}
