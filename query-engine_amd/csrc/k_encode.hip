// Result encoding after the path: PostgreSQL DataRow
// messages in text format, as the reference's pgwire front end builds them
// (crates/query-pgwire/src/result.rs:56-176: one DataRowEncoder per row,
// encode_value per cell; pgwire 0.28.0 renders each value with Rust's
// Display, fmt_float.h).  Message: 'D', Int32 length (self-inclusive), Int16
// field count, then per field Int32 length (-1 = NULL) and the text, all
// big-endian.
//
// Two passes over the rows: every thread measures its row (the formatter
// runs in length-only mode), an exclusive scan places the rows, and the same
// code writes them.  The output is one Utf8 column whose i-th string is row
// i's complete DataRow message, so the buffer can go to the socket as is.
//
// Date32 / Date64 / Timestamp cells (result.rs:146-172) are rendered from their physical integers:
// the civil date by the era / day-of-era arithmetic (no loops, no tables), the time of day and the
// fraction by integer division.  This restates the published behaviour of chrono's NaiveDate /
// NaiveDateTime formatting and of arrow-cast 53.4.1's array_value_to_string; neither crate is
// vendored here, so parity with them is unpinned, as for pgwire's float text.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "device_common.h"
#include "fmt_float.h"
#include "ops.h"

namespace qeh {

constexpr int kEncMaxCols = 32;

struct EncCol {
    ColRef c;             // (a temporal column: its physical Int32 / Int64)
    const int32_t *offs;  // Utf8: offsets (already advanced by the column offset)
    const uint8_t *data;
    int32_t temporal;     // the column's temporal qeh_dtype, 0 for every other column
};
struct EncCols {
    EncCol col[kEncMaxCols];
    int32_t n;
};

__device__ inline void put_be32(char *p, int32_t v) {
    p[0] = (char)((uint32_t)v >> 24);
    p[1] = (char)((uint32_t)v >> 16);
    p[2] = (char)((uint32_t)v >> 8);
    p[3] = (char)(uint32_t)v;
}

// Days since 1970-01-01 of the years 0000 and 9999's ends (proleptic Gregorian): chrono prints a
// year outside them in a signed five-digit form, which is not rendered here.
constexpr int64_t kDayMin = -719528, kDayMax = 2932896;

// a = q * b + r with 0 <= r < b (b > 0): the quotient floors towards -inf, nothing overflows
__device__ inline int64_t floor_divmod(int64_t a, int64_t b, int64_t *r) {
    int64_t q = a / b, m = a % b;
    if (m < 0) m += b, q -= 1;
    *r = m;
    return q;
}

__device__ inline void put_dec(char *p, uint32_t v, int digits) {
    for (int i = digits - 1; i >= 0; --i, v /= 10u) p[i] = (char)('0' + v % 10u);
}

// YYYY-MM-DD of `days` in [kDayMin, kDayMax]: civil-from-days by era (400 years = 146097 days) and
// day of era, the year counted from March so that the leap day is the last of its year.  One era
// is added before the division so that everything is unsigned; it comes off the year again.
__device__ inline void put_date(char *p, int32_t days) {
    const uint32_t z = (uint32_t)(days + 719468 + 146097);
    const uint32_t era = z / 146097u;
    const uint32_t doe = z - era * 146097u;                                           // [0, 146096]
    const uint32_t yoe = (doe - doe / 1460u + doe / 36524u - doe / 146096u) / 365u;  // [0, 399]
    const uint32_t doy = doe - (365u * yoe + yoe / 4u - yoe / 100u);                  // [0, 365], from 1 March
    const uint32_t mp = (5u * doy + 2u) / 153u;                                       // [0, 11], March = 0
    const uint32_t d = doy - (153u * mp + 2u) / 5u + 1u;
    const uint32_t m = mp < 10u ? mp + 3u : mp - 9u;
    const uint32_t y = yoe + era * 400u - 400u + (m <= 2u ? 1u : 0u);
    put_dec(p, y, 4);
    p[4] = '-';
    put_dec(p + 5, m, 2);
    p[7] = '-';
    put_dec(p + 8, d, 2);
}

// text of one temporal cell (the row is valid); `bad` is set for a year outside 0000-9999, whose
// cell is left empty
__device__ inline int enc_temporal(const EncCol &e, int64_t row, char *out, uint32_t &bad) {
    const int64_t v = load_i64(e.c, row);
    int64_t secs = 0, rem = 0;
    uint32_t nanos = 0;
    switch (e.temporal) {
        case QEH_DT_DATE32:  // NaiveDate::from_num_days_from_ce_opt(days + 719163)
            if (v < kDayMin || v > kDayMax) {
                bad = 1u;
                return 0;
            }
            if (out) put_date(out, (int32_t)v);
            return 10;
        case QEH_DT_DATE64: {
            // result.rs:155-166: secs = ms / 1000 truncating, nsecs = ((ms % 1000) * 1_000_000) as u32,
            // which wraps past 2e9 for a negative remainder: from_timestamp is None and the cell is
            // the text "NULL"
            if (v < 0 && v % 1000 != 0) {
                if (out) out[0] = 'N', out[1] = 'U', out[2] = 'L', out[3] = 'L';
                return 4;
            }
            int64_t sod;
            const int64_t days = floor_divmod(v / 1000, 86400, &sod);
            if (days < kDayMin || days > kDayMax) {
                bad = 1u;
                return 0;
            }
            if (out) put_date(out, (int32_t)days);
            return 10;
        }
        case QEH_DT_TIMESTAMP_S: secs = v; break;
        case QEH_DT_TIMESTAMP_MS:
            secs = floor_divmod(v, 1000, &rem);
            nanos = (uint32_t)rem * 1000000u;
            break;
        case QEH_DT_TIMESTAMP_US:
            secs = floor_divmod(v, 1000000, &rem);
            nanos = (uint32_t)rem * 1000u;
            break;
        default:
            secs = floor_divmod(v, 1000000000, &rem);
            nanos = (uint32_t)rem;
            break;
    }
    // chrono's NaiveDateTime Debug: the fraction only when non-zero, in 3, 6 or 9 digits
    const int64_t days = floor_divmod(secs, 86400, &rem);  // rem: the second of the day
    if (days < kDayMin || days > kDayMax) {
        bad = 1u;
        return 0;
    }
    const int frac = nanos == 0 ? 0 : nanos % 1000000u == 0 ? 3 : nanos % 1000u == 0 ? 6 : 9;
    if (out) {
        const uint32_t sod = (uint32_t)rem;
        put_date(out, (int32_t)days);
        out[10] = 'T';
        put_dec(out + 11, sod / 3600u, 2);
        out[13] = ':';
        put_dec(out + 14, sod / 60u % 60u, 2);
        out[16] = ':';
        put_dec(out + 17, sod % 60u, 2);
        if (frac) {
            out[19] = '.';
            put_dec(out + 20, frac == 3 ? nanos / 1000000u : frac == 6 ? nanos / 1000u : nanos, frac);
        }
    }
    return 19 + (frac ? 1 + frac : 0);
}

// text of one cell at out (nullptr: length only); -1 for NULL
__device__ inline int enc_cell(const EncCol &e, int64_t row, char *out, uint32_t &bad) {
    if (!col_valid(e.c, row)) return -1;
    if (e.temporal) return enc_temporal(e, row, out, bad);
    switch (e.c.dtype) {
        case QEH_DT_BOOL:
            if (out) out[0] = bit_at((const uint8_t *)e.c.values, e.c.vbit0 + row) ? 't' : 'f';
            return 1;
        case QEH_DT_INT32: case QEH_DT_INT64: case QEH_DT_UINT32:
            return fmt_i64(out, load_i64(e.c, row));
        case QEH_DT_FLOAT32:
            return fmt_f32(out, ((const float *)e.c.values)[row]);
        case QEH_DT_FLOAT64:
            return fmt_f64(out, ((const double *)e.c.values)[row]);
        case QEH_DT_UTF8: {
            const int32_t s = e.offs[row], t = e.offs[row + 1];
            if (out)
                for (int32_t i = s; i < t; ++i) out[i - s] = (char)e.data[i];
            return t - s;
        }
        default: return 0;
    }
}

// `flag` (may be nullptr): set when a non-NULL temporal cell's year lies outside 0000-9999 -- one
// OR per lane, one atomic per wave
__global__ void k_pg_row_len(EncCols cols, int64_t n, uint32_t *__restrict__ len, uint32_t *__restrict__ flag) {
    uint32_t bad = 0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
        uint32_t l = 1 + 4 + 2;
        for (int j = 0; j < cols.n; ++j) {
            const int c = enc_cell(cols.col[j], r, nullptr, bad);
            l += 4 + (c > 0 ? (uint32_t)c : 0u);
        }
        len[r] = l;
    }
    if (__ballot(bad != 0) != 0 && (threadIdx.x & 63) == 0 && flag) atomicOr(flag, 1u);
}

__device__ inline void pg_write_row(const EncCols &cols, int64_t r, char *p, uint32_t bytes) {
    p[0] = 'D';
    put_be32(p + 1, (int32_t)(bytes - 1));
    p[5] = (char)(cols.n >> 8);
    p[6] = (char)cols.n;
    char *q = p + 7;
    uint32_t bad = 0;  // (the length pass has reported it: no row is written then)
    for (int j = 0; j < cols.n; ++j) {
        const int c = enc_cell(cols.col[j], r, q + 4, bad);
        put_be32(q, c);
        q += 4 + (c > 0 ? c : 0);
    }
}

// One workgroup per 256 rows: the rows are rendered into LDS at their relative offsets, then the
// workgroup's contiguous byte range leaves with coalesced 4-byte stores (a row-per-thread direct
// write would scatter ~50-byte pieces).  Ranges larger than the LDS stage are written directly.
// LDS = the stage's bytes: 16 KB (rows averaging <= 56 B: more workgroups per CU for the formatting
// work; a workgroup whose rows overflow it writes directly) or 48 KB.  The choice is made from the
// measured total, so it holds for temporal cells as it stands: a date cell is at most 4 + 10 B and a
// timestamp cell at most 4 + 29 B, so e.g. {Int64, Date32, Timestamp(us)} rows reach 7 + 24 + 14 + 30 =
// 75 B and take the 48 KB stage (256 rows <= 19200 B), {Int64, Date32} rows at most 45 B the 16 KB one.
template <int LDS>
__global__ __launch_bounds__(kBlock, 6) void k_pg_row_write(EncCols cols, int64_t n, const uint64_t *__restrict__ at,
                                                         const uint32_t *__restrict__ len, char *__restrict__ out,
                                                         int32_t *__restrict__ out_offs, uint64_t total) {
    constexpr int kEncLds = LDS;
    __shared__ __attribute__((aligned(16))) char stage[kEncLds + 16];
    for (int64_t b0 = (int64_t)blockIdx.x * kBlock; b0 < n; b0 += (int64_t)gridDim.x * kBlock) {
        const int64_t r = b0 + threadIdx.x;
        const uint64_t base = at[b0];
        const uint64_t end = b0 + kBlock < n ? at[b0 + kBlock] : total;
        const uint64_t span = end - base;
        if (r < n) out_offs[r] = (int32_t)at[r];
        if (r == n - 1) out_offs[n] = (int32_t)total;
        if (span > (uint64_t)kEncLds) {  // wide rows: direct
            if (r < n) pg_write_row(cols, r, out + at[r], len[r]);
            continue;
        }
        // stage at the destination's 16-B alignment so that whole 16-B pieces can be stored
        const uint32_t lead = (uint32_t)(base & 15);
        if (r < n) pg_write_row(cols, r, stage + lead + (at[r] - base), len[r]);
        __syncthreads();
        const uint32_t head = lead ? 16 - lead : 0;  // bytes before the first aligned 16-B piece
        const uint32_t h = (uint32_t)(head < span ? head : span);
        if (threadIdx.x < h) out[base + threadIdx.x] = stage[lead + threadIdx.x];
        const uint32_t body = (uint32_t)(span - h) / 16;
        typedef unsigned int v4u __attribute__((ext_vector_type(4)));
        v4u *dst = (v4u *)(out + base + h);
        const v4u *src = (const v4u *)(stage + lead + h);
        for (uint32_t i = threadIdx.x; i < body; i += kBlock) dst[i] = src[i];
        for (uint32_t i = h + body * 16 + threadIdx.x; i < span; i += kBlock) out[base + i] = stage[lead + i];
        __syncthreads();
    }
}

}  // namespace qeh

using namespace qeh;

extern "C" int qeh_encode_pg_datarows(qeh_ctx *ctx, const qeh_column *cols, int n_cols, qeh_column *out) {
    if (!ctx || !out || n_cols < 0 || (n_cols > 0 && !cols)) return fail(QEH_E_INVALID, "qeh_encode_pg_datarows: bad argument");
    if (n_cols > kEncMaxCols) return fail(QEH_E_UNSUPPORTED, "DataRow encoding: at most 32 columns per call");
    DeviceGuard dg(ctx->device);
    std::memset(out, 0, sizeof(*out));
    const int64_t n = n_cols > 0 ? cols[0].length : 0;
    EncCols ec{};
    ec.n = n_cols;
    for (int j = 0; j < n_cols; ++j) {
        QEH_TRY(check_column(cols[j], "encode"));
        if (cols[j].length != n) return fail(QEH_E_INVALID, "encode: columns have different lengths");
        switch (cols[j].dtype) {
            case QEH_DT_BOOL: case QEH_DT_INT32: case QEH_DT_INT64: case QEH_DT_UINT32: case QEH_DT_FLOAT32:
            case QEH_DT_FLOAT64: case QEH_DT_UTF8: break;
            case QEH_DT_DATE32: case QEH_DT_DATE64: case QEH_DT_TIMESTAMP_S: case QEH_DT_TIMESTAMP_MS:
            case QEH_DT_TIMESTAMP_US: case QEH_DT_TIMESTAMP_NS:
                ec.col[j].temporal = cols[j].dtype;
                break;
            default: return fail(QEH_E_UNSUPPORTED, "encode: unsupported column type");
        }
        ec.col[j].c = make_colref(cols[j]);
        if (cols[j].dtype == QEH_DT_UTF8) {
            ec.col[j].offs = cols[j].offsets + cols[j].offset;
            ec.col[j].data = (const uint8_t *)cols[j].values;
        }
    }
    DevBuf len, at, flag;  // flag: only when a temporal column can raise it
    if (any_temporal(cols, n_cols)) {
        QEH_TRY(flag.alloc(ctx, 8));
        QEH_HIP(hipMemsetAsync(flag.p, 0, 8, ctx->stream));
    }
    QEH_TRY(len.alloc(ctx, (size_t)std::max<int64_t>(n, 1) * 4));
    QEH_TRY(at.alloc(ctx, (size_t)std::max<int64_t>(n, 1) * 8));
    const int grid = grid_for(ctx, n, kBlock, 8);
    uint64_t total = 0;
    if (n > 0) {
        KernelTimer kt(ctx, "encode_len");
        hipLaunchKernelGGL(k_pg_row_len, dim3(grid), dim3(kBlock), 0, ctx->stream, ec, n, len.as<uint32_t>(), flag.as<uint32_t>());
    }
    QEH_HIP(hipGetLastError());
    QEH_TRY(exclusive_scan_u32(ctx, len.as<uint32_t>(), at.as<uint64_t>(), n, &total));
    if (flag.p && n > 0) {
        uint32_t bad = 0;
        QEH_TRY(read_small(ctx, &bad, flag.p, 4));
        if (bad)  // chrono's signed five-digit years (and None past +-262143) are not rendered: the CPU encodes this batch
            return fail(QEH_E_UNSUPPORTED, "DataRow encoding: date or timestamp year outside 0000-9999");
    }
    if (total > 0x7FFFFFFFull)
        return fail(QEH_E_UNSUPPORTED, "DataRow encoding beyond 2 GiB per call: encode the batch in slices");
    out->dtype = QEH_DT_UTF8;
    out->owned = 1;
    out->length = n;
    void *o = nullptr, *d = nullptr;
    QEH_TRY(ctx->pool->alloc((size_t)(n + 1) * 4, &o));
    int s = ctx->pool->alloc(std::max<size_t>((size_t)total, 8), &d);
    if (s != QEH_OK) {
        ctx->pool->free(o);
        return s;
    }
    out->offsets = (int32_t *)o;
    out->values = d;
    out->values_bytes = (int64_t)total;
    if (n == 0) QEH_HIP(hipMemsetAsync(o, 0, 4, ctx->stream));
    else {
        KernelTimer kt(ctx, "encode_write");
        const char *ek = std::getenv("QEH_ENC_LDS_KB");  // (A/B)
        const bool small = ek ? atoi(ek) == 16 : total <= (uint64_t)n * 56;
        auto wk = small ? k_pg_row_write<16 * 1024> : k_pg_row_write<48 * 1024>;
        hipLaunchKernelGGL(wk, dim3(grid), dim3(kBlock), 0, ctx->stream, ec, n, at.as<uint64_t>(),
                           len.as<uint32_t>(), (char *)d, (int32_t *)o, total);
    }
    QEH_HIP(hipGetLastError());
    QEH_HIP(hipStreamSynchronize(ctx->stream));
    return QEH_OK;
}
