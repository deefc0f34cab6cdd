// Scalar functions in expressions: PhysicalExpr::ScalarFunction (physical_plan.rs:112-116) as
// evaluate_scalar_function computes it (crates/query-executor/src/operators.rs:64-259).
//
// The register interpreter (expr_device.h) is inlined into every fused kernel and stays as it is:
// a function is materialised at its boundary instead.  rewrite_scalar_functions walks the postfix
// once, innermost function first; each argument that is not a leaf goes through qeh_eval into a
// temporary, the function's kernel writes a temporary column appended after the operator's inputs,
// and the subtree becomes a COLUMN leaf.  What remains (arithmetic, comparisons, Utf8 comparisons
// of the new leaves) takes the existing paths.  The same walk replaces every full-text match
// (QEH_OP_TSMATCH over operands that may be wrapped in TO_TSVECTOR / TO_TSQUERY) by the BOOL column
// of k_ts_match.hip: the wrapping function is peeled into its side's mode, nothing is materialised.
//
// Kernels (each under its own KernelTimer name):
//   scalar_math      ABS / CEIL / FLOOR / ROUND / SQRT / POWER over 8-byte slots, two rows per lane
//                    (16-B loads and stores), validity words by ballot
//   str_length       LENGTH: offsets -> Int64
//   str_case_stream  UPPER / LOWER of a column without NULLs: its byte slice as one flat stream,
//                    16-B vectors, SWAR range test per dword; the output keeps the input's
//                    position within a 16-B line (its offsets start at that many bytes), so loads
//                    and stores are aligned together and only a head and a tail go bytewise
//   str_rebase_offsets  the offsets of that output
//   str_row_len / str_rows  the general path: UPPER / LOWER of a nullable column and CONCAT of k
//                    operands (column or literal): per-row output lengths, exclusive scan, then the
//                    bytes, driven by output position (one 16-B store per lane, contiguous per wave)
// UPPER / LOWER map ASCII letters only; any byte >= 0x80 in a non-NULL row sets a flag (one atomic
// per wave) and the call returns QEH_E_UNSUPPORTED: Rust's to_uppercase / to_lowercase are full
// Unicode and can change lengths.
#include <algorithm>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "device_common.h"
#include "ops.h"

namespace qeh {

// ---- numeric -------------------------------------------------------------------------------
struct MathArg {
    const int64_t *v;      // 8-byte slots, advanced by the column offset
    const uint8_t *valid;  // nullptr = all valid
    int64_t vbit0;
};

__device__ __forceinline__ bool arg_valid(const MathArg &a, int64_t row) {
    return a.valid == nullptr || bit_at(a.valid, a.vbit0 + row);
}

// One slot.  Int64 ABS wraps at INT64_MIN like a release build's i64::abs; the Float64 functions are
// the correctly rounded / exact IEEE operations Rust's f64 methods map to (round: half away from zero).
__device__ __forceinline__ int64_t math_slot(int func, bool is_int, int64_t x, int64_t y) {
    if (is_int) return x < 0 ? (int64_t)(0ull - (uint64_t)x) : x;
    const double d = as_f64(x);
    double r;
    switch (func) {
        case QEH_FN_ABS: r = fabs(d); break;
        case QEH_FN_CEIL: r = ceil(d); break;
        case QEH_FN_FLOOR: r = floor(d); break;
        case QEH_FN_ROUND: r = round(d); break;
        case QEH_FN_SQRT: r = sqrt(d); break;
        default: r = pow(d, as_f64(y)); break;  // QEH_FN_POWER
    }
    return f64_bits(r);
}

// bit i of x -> bit 2 i
__device__ __forceinline__ uint64_t spread_bits(uint32_t x) {
    uint64_t v = x;
    v = (v | (v << 16)) & 0x0000FFFF0000FFFFull;
    v = (v | (v << 8)) & 0x00FF00FF00FF00FFull;
    v = (v | (v << 4)) & 0x0F0F0F0F0F0F0F0Full;
    v = (v | (v << 2)) & 0x3333333333333333ull;
    v = (v | (v << 1)) & 0x5555555555555555ull;
    return v;
}

// A wave takes 128 consecutive rows, lane l rows 2 l and 2 l + 1.  ALIGNED: the inputs' row 0 is
// 16-B aligned, so a pair is one 16-B load; the output (a fresh allocation) always is.
template <bool ALIGNED>
__global__ __launch_bounds__(kBlock) void k_scalar_math(int func, int is_int, MathArg a, MathArg b, int64_t n,
                                                        int64_t *__restrict__ out, uint64_t *__restrict__ out_valid) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * (blockDim.x / 64);
    for (int64_t w = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); w * 128 < n; w += nw) {
        const int64_t base = w * 128, r0 = base + 2 * lane;
        const bool live0 = r0 < n, live1 = r0 + 1 < n;
        int64_t x0 = 0, x1 = 0, y0 = 0, y1 = 0;
        if (ALIGNED && live1) {
            const longlong2 t = *reinterpret_cast<const longlong2 *>(a.v + r0);
            x0 = t.x, x1 = t.y;
            if (b.v) {
                const longlong2 u = *reinterpret_cast<const longlong2 *>(b.v + r0);
                y0 = u.x, y1 = u.y;
            }
        } else {
            if (live0) x0 = a.v[r0];
            if (live1) x1 = a.v[r0 + 1];
            if (b.v && live0) y0 = b.v[r0];
            if (b.v && live1) y1 = b.v[r0 + 1];
        }
        const int64_t z0 = math_slot(func, is_int != 0, x0, y0), z1 = math_slot(func, is_int != 0, x1, y1);
        if (live1) {
            longlong2 t;
            t.x = z0, t.y = z1;
            *reinterpret_cast<longlong2 *>(out + r0) = t;
        } else if (live0) {
            out[r0] = z0;
        }
        if (out_valid) {
            const bool v0 = live0 && arg_valid(a, r0) && (!b.v || arg_valid(b, r0));
            const bool v1 = live1 && arg_valid(a, r0 + 1) && (!b.v || arg_valid(b, r0 + 1));
            const uint64_t e = __ballot(v0), o = __ballot(v1);  // lane l: rows base + 2 l, base + 2 l + 1
            if (lane == 0) {
                out_valid[2 * w] = spread_bits((uint32_t)e) | (spread_bits((uint32_t)o) << 1);
                if (base + 64 < n) out_valid[2 * w + 1] = spread_bits((uint32_t)(e >> 32)) | (spread_bits((uint32_t)(o >> 32)) << 1);
            }
        }
    }
}

// ---- strings -------------------------------------------------------------------------------
__global__ void k_str_length(const int32_t *__restrict__ offs, ColRef valid, int64_t n, int64_t *__restrict__ out,
                             uint64_t *__restrict__ out_valid) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * (blockDim.x / 64);
    for (int64_t w = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); w * 64 < n; w += nw) {
        const int64_t i = w * 64 + lane;
        if (i < n) out[i] = (int64_t)(offs[i + 1] - offs[i]);
        if (out_valid) {
            const uint64_t vb = __ballot(i < n && col_valid(valid, i));
            if (lane == 0) out_valid[w] = vb;
        }
    }
}

// ASCII case mapping of the four bytes of x at once.  With the high bits masked off, adding
// 0x80 - lo carries into a byte's high bit exactly when the byte is >= lo, and no sum passes 0xFF,
// so bytes do not disturb each other.  Bytes in [first, last] get bit 5 flipped; bytes >= 0x80 are
// left alone (the caller refuses them).
template <bool LOWER>
__device__ __forceinline__ uint32_t case_dword(uint32_t x) {
    constexpr uint32_t first = LOWER ? 'A' : 'a', last = LOWER ? 'Z' : 'z';
    constexpr uint32_t ones = 0x01010101u;
    const uint32_t t = x & 0x7F7F7F7Fu;
    const uint32_t ge_first = t + (0x80u - first) * ones;
    const uint32_t gt_last = t + (0x80u - (last + 1)) * ones;
    const uint32_t hit = ge_first & ~gt_last & ~x & 0x80808080u;
    return x ^ (hit >> 2);
}

template <bool LOWER>
__device__ __forceinline__ uint8_t case_byte(uint8_t c) {
    if (LOWER) return (c >= 'A' && c <= 'Z') ? (uint8_t)(c + 32) : c;
    return (c >= 'a' && c <= 'z') ? (uint8_t)(c - 32) : c;
}

// in[0, len) -> out[0, len); in and out share their position within a 16-B line.  `head` bytes
// lead up to the first line boundary (head <= len); whole lines follow; the rest is the tail.
template <bool LOWER>
__global__ __launch_bounds__(kBlock) void k_str_case_stream(const uint8_t *__restrict__ in, uint8_t *__restrict__ out,
                                                            int64_t len, int head, uint32_t *__restrict__ flag) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    const int64_t nvec = (len - head) >> 4;
    const uint4 *__restrict__ vin = reinterpret_cast<const uint4 *>(in + head);
    uint4 *__restrict__ vout = reinterpret_cast<uint4 *>(out + head);
    uint32_t acc = 0;
    for (int64_t v = gid; v < nvec; v += stride) {
        uint4 x = vin[v];
        acc |= x.x | x.y | x.z | x.w;
        x.x = case_dword<LOWER>(x.x);
        x.y = case_dword<LOWER>(x.y);
        x.z = case_dword<LOWER>(x.z);
        x.w = case_dword<LOWER>(x.w);
        vout[v] = x;
    }
    const int64_t tail0 = head + (nvec << 4);
    const int edge = head + (int)(len - tail0);  // < 32 bytes outside whole lines
    if (gid < edge) {
        const int64_t p = gid < head ? gid : tail0 + (gid - head);
        const uint8_t c = in[p];
        acc |= c;
        out[p] = case_byte<LOWER>(c);
    }
    if (__ballot((acc & 0x80808080u) != 0) != 0 && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

__global__ void k_str_rebase_offsets(const int32_t *__restrict__ offs, int64_t n, int32_t delta, int32_t *__restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (int64_t)gridDim.x * blockDim.x)
        out[i] = offs[i] + delta;
}

constexpr int kMaxStrOps = 8;  // operands of one str_rows pass (CONCAT over more is folded)
struct StrOperand {
    const int32_t *offs;  // column: offsets advanced by the column offset
    const uint8_t *data;  // column bytes, or the literal's bytes
    int32_t lit_len;
    int32_t is_lit;
};
enum { STR_CONCAT = 0, STR_UPPER = 1, STR_LOWER = 2 };
struct StrOperands {
    StrOperand op[kMaxStrOps];
    int32_t k;
    int32_t mode;
    ColRef valid;  // UPPER / LOWER: the column's validity (a NULL row's output slot is empty)
};

__device__ __forceinline__ int64_t slot_len(const StrOperand &o, int64_t row) {
    const int32_t l = o.is_lit ? o.lit_len : o.offs[row + 1] - o.offs[row];
    return l > 0 ? l : 0;
}
__device__ __forceinline__ const uint8_t *slot_ptr(const StrOperand &o, int64_t row) {
    return o.is_lit ? o.data : o.data + o.offs[row];
}

// Output bytes per row (saturating: anything near 2^31 fails the total's check) and, for UPPER /
// LOWER, the result's validity words.  CONCAT reads every slot, whatever its validity.
__global__ void k_str_row_len(StrOperands ops, int64_t n, uint32_t *__restrict__ len, uint64_t *__restrict__ out_valid) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * (blockDim.x / 64);
    for (int64_t w = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); w * 64 < n; w += nw) {
        const int64_t i = w * 64 + lane;
        const bool v = i < n && col_valid(ops.valid, i);
        if (i < n) {
            uint64_t s = 0;
            if (ops.mode == STR_CONCAT || v)
                for (int j = 0; j < ops.k; ++j) s += (uint64_t)slot_len(ops.op[j], i);
            len[i] = (uint32_t)(s < 0x80000000ull ? s : 0x80000000ull);
        }
        if (out_valid) {
            const uint64_t vb = __ballot(v);
            if (lane == 0) out_valid[w] = vb;
        }
    }
}

// The bytes, by output position: a lane owns 16 consecutive output bytes, finds the row holding the
// first of them in the scanned lengths (excl[0 .. n), total) and walks operands and rows from there.
// Also turns the scan into the result's int32 offsets.
__global__ __launch_bounds__(kBlock) void k_str_rows_write(StrOperands ops, int64_t n, const uint64_t *__restrict__ excl,
                                                           uint64_t total, uint8_t *__restrict__ out,
                                                           int32_t *__restrict__ out_offs, uint32_t *__restrict__ flag) {
    const int64_t gid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = gid; i <= n; i += stride) out_offs[i] = (int32_t)(i < n ? excl[i] : total);
    const int64_t nchunks = (int64_t)((total + 15) >> 4);
    uint32_t acc = 0;
    for (int64_t c = gid; c < nchunks; c += stride) {
        const uint64_t p0 = (uint64_t)c << 4;
        int cnt = (int)(total - p0 < 16 ? total - p0 : 16);
        int64_t lo = 0, hi = n;  // excl[lo] <= p0 < excl[hi] (excl[n] = total)
        while (hi - lo > 1) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (excl[mid] <= p0) lo = mid;
            else hi = mid;
        }
        int64_t row = lo;  // the last row starting at or before p0: the one holding byte p0
        int64_t q = (int64_t)(p0 - excl[row]);
        int j = 0;
        int64_t l = slot_len(ops.op[0], row);
        const uint8_t *src = slot_ptr(ops.op[0], row);
        uint32_t w[4] = {0, 0, 0, 0};
#pragma unroll
        for (int b = 0; b < 16; ++b) {
            if (b < cnt) {
                // output bytes remain, so a later non-empty slot of a row that is written exists
                // (the lengths were summed from these same slots); the row bound only keeps a
                // lane inside the inputs should the offsets not be monotone
                while (q >= l) {
                    q -= l;
                    if (++j == ops.k) {
                        j = 0;
                        ++row;
                        if (ops.mode != STR_CONCAT)
                            while (row < n && !col_valid(ops.valid, row)) ++row;
                    }
                    if (row >= n) {
                        cnt = b;
                        break;
                    }
                    l = slot_len(ops.op[j], row);
                    src = slot_ptr(ops.op[j], row);
                }
            }
            if (b < cnt) {
                uint8_t ch = src[q++];
                if (ops.mode != STR_CONCAT) {
                    acc |= ch;
                    ch = ops.mode == STR_LOWER ? case_byte<true>(ch) : case_byte<false>(ch);
                }
                w[b >> 2] |= (uint32_t)ch << (8 * (b & 3));
            }
        }
        uint4 x;
        x.x = w[0], x.y = w[1], x.z = w[2], x.w = w[3];
        *reinterpret_cast<uint4 *>(out + p0) = x;  // the buffer is padded to whole 16-B chunks
    }
    if (__ballot((acc & 0x80u) != 0) != 0 && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}

// ---- host: one function over materialised arguments ------------------------------------------
namespace {

bool has_nulls(const qeh_column &c) { return c.validity && c.null_count != 0; }

// An owned Utf8 column of n rows: offsets (n + 1 entries) and `bytes` value bytes (padded to whole
// 16-B chunks), uninitialised.
int alloc_utf8(qeh_ctx *ctx, int64_t n, uint64_t bytes, bool with_validity, qeh_column *out) {
    std::memset(out, 0, sizeof(*out));
    void *o = nullptr, *d = nullptr, *v = nullptr;
    QEH_TRY(ctx->pool->alloc((size_t)(n + 1) * 4, &o));
    int s = ctx->pool->alloc((size_t)((bytes + 15) & ~15ull) + 16, &d);
    if (s == QEH_OK && with_validity) s = ctx->pool->alloc(std::max<size_t>(((size_t)(n + 63) / 64) * 8, 8), &v);
    if (s != QEH_OK) {
        ctx->pool->free(o);
        if (d) ctx->pool->free(d);
        return s;
    }
    out->dtype = QEH_DT_UTF8;
    out->owned = 1;
    out->length = n;
    out->null_count = with_validity ? -1 : 0;
    out->values = d;
    out->validity = (uint8_t *)v;
    out->offsets = (int32_t *)o;
    out->values_bytes = (int64_t)bytes;
    return QEH_OK;
}

int non_ascii(const char *fname) {
    return fail(QEH_E_UNSUPPORTED, std::string(fname) + ": non-ASCII input (a byte >= 0x80 in a non-NULL row); the device "
                                       "maps ASCII letters only, Unicode case mapping can change lengths");
}

int scalar_math(qeh_ctx *ctx, int func, const qeh_column &a, const qeh_column *b, int64_t n, qeh_column *out) {
    QEH_TRY(check_column(a, "scalar function argument"));
    if (b) QEH_TRY(check_column(*b, "scalar function argument"));
    const bool nullable = has_nulls(a) || (b && has_nulls(*b));
    QEH_TRY(alloc_column(ctx, a.dtype, n, nullable, out));
    if (n == 0) return QEH_OK;
    auto arg = [](const qeh_column &c) {
        MathArg m{};
        m.v = (const int64_t *)c.values + c.offset;
        if (has_nulls(c)) m.valid = c.validity, m.vbit0 = c.offset;
        return m;
    };
    const MathArg ma = arg(a), mb = b ? arg(*b) : MathArg{};
    const bool aligned = (((uintptr_t)ma.v | (uintptr_t)mb.v) & 15) == 0;
    const int grid = grid_for(ctx, (n + 127) / 128, kBlock / 64, 8);
    {
        KernelTimer kt(ctx, "scalar_math");
        if (aligned)
            hipLaunchKernelGGL(k_scalar_math<true>, dim3(grid), dim3(kBlock), 0, ctx->stream, func, a.dtype == QEH_DT_INT64, ma,
                               mb, n, (int64_t *)out->values, (uint64_t *)out->validity);
        else
            hipLaunchKernelGGL(k_scalar_math<false>, dim3(grid), dim3(kBlock), 0, ctx->stream, func, a.dtype == QEH_DT_INT64,
                               ma, mb, n, (int64_t *)out->values, (uint64_t *)out->validity);
    }
    QEH_HIP(hipGetLastError());
    return QEH_OK;
}

int str_length(qeh_ctx *ctx, const qeh_column &c, int64_t n, qeh_column *out) {
    QEH_TRY(check_column(c, "LENGTH"));
    QEH_TRY(alloc_column(ctx, QEH_DT_INT64, n, has_nulls(c), out));
    if (n == 0) return QEH_OK;
    {
        KernelTimer kt(ctx, "str_length");
        hipLaunchKernelGGL(k_str_length, dim3(grid_for(ctx, (n + 63) / 64, kBlock / 64, 8)), dim3(kBlock), 0, ctx->stream,
                           c.offsets + c.offset, make_colref(c), n, (int64_t *)out->values, (uint64_t *)out->validity);
    }
    QEH_HIP(hipGetLastError());
    return QEH_OK;
}

// UPPER / LOWER of a column without NULLs: rows [offset, offset + n) own the contiguous bytes
// [offsets[offset], offsets[offset + n)), mapped as one stream.
int str_case_stream(qeh_ctx *ctx, int func, const qeh_column &c, int64_t n, qeh_column *out) {
    int32_t b0 = 0, b1 = 0;
    if (n > 0) {
        QEH_TRY(read_small(ctx, &b0, c.offsets + c.offset, 4));
        QEH_TRY(read_small(ctx, &b1, c.offsets + c.offset + n, 4));
    }
    if (b1 < b0 || b0 < 0) return fail(QEH_E_INVALID, std::string(scalar_fn_name(func)) + ": malformed Utf8 offsets");
    const int64_t len = (int64_t)b1 - b0;
    const uint8_t *in = (const uint8_t *)c.values + b0;
    const int mis = (int)((uintptr_t)in & 15);  // the output starts as deep into a 16-B line as the input
    QEH_TRY(alloc_utf8(ctx, n, (uint64_t)(mis + len), false, out));
    void *scr = nullptr;
    int s = scratch_zeroed(ctx, 64, &scr);
    if (s == QEH_OK && len > 0) {
        const int head = (int)std::min<int64_t>(len, (16 - mis) & 15);
        const int grid = grid_for(ctx, std::max<int64_t>((len - head) >> 4, 32), kBlock, 8);
        KernelTimer kt(ctx, "str_case_stream");
        if (func == QEH_FN_LOWER)
            hipLaunchKernelGGL(k_str_case_stream<true>, dim3(grid), dim3(kBlock), 0, ctx->stream, in,
                               (uint8_t *)out->values + mis, len, head, (uint32_t *)scr);
        else
            hipLaunchKernelGGL(k_str_case_stream<false>, dim3(grid), dim3(kBlock), 0, ctx->stream, in,
                               (uint8_t *)out->values + mis, len, head, (uint32_t *)scr);
    }
    if (s == QEH_OK) {
        KernelTimer kt(ctx, "str_rebase_offsets");
        if (n > 0)
            hipLaunchKernelGGL(k_str_rebase_offsets, dim3(grid_for(ctx, n + 1, kBlock * 4, 8)), dim3(kBlock), 0, ctx->stream,
                               c.offsets + c.offset, n, (int32_t)(mis - b0), out->offsets);
        else if (hipMemsetAsync(out->offsets, 0, 4, ctx->stream) != hipSuccess)
            s = fail(QEH_E_HIP, "hipMemsetAsync failed");
    }
    if (s == QEH_OK && hipGetLastError() != hipSuccess) s = fail(QEH_E_HIP, "UPPER / LOWER: kernel launch failed");
    uint32_t flag = 0;
    if (s == QEH_OK) s = read_small(ctx, &flag, scr, 4);
    if (s == QEH_OK && flag) s = non_ascii(scalar_fn_name(func));
    if (s != QEH_OK) qeh_column_release(ctx, out);
    return s;
}

// The general string path: per-row lengths, scan, bytes by output position.
int str_rows(qeh_ctx *ctx, const StrOperands &ops, int64_t n, bool nullable, const char *fname, qeh_column *out) {
    DevBuf len, excl;
    QEH_TRY(len.alloc(ctx, (size_t)std::max<int64_t>(n, 1) * 4));
    QEH_TRY(excl.alloc(ctx, (size_t)std::max<int64_t>(n, 1) * 8));
    DevBuf valid;
    if (nullable) QEH_TRY(valid.alloc(ctx, std::max<size_t>(((size_t)(n + 63) / 64) * 8, 8)));
    if (n > 0) {
        KernelTimer kt(ctx, "str_row_len");
        hipLaunchKernelGGL(k_str_row_len, dim3(grid_for(ctx, (n + 63) / 64, kBlock / 64, 8)), dim3(kBlock), 0, ctx->stream, ops,
                           n, len.as<uint32_t>(), nullable ? valid.as<uint64_t>() : nullptr);
    }
    QEH_HIP(hipGetLastError());
    uint64_t total = 0;
    QEH_TRY(exclusive_scan_u32(ctx, len.as<uint32_t>(), excl.as<uint64_t>(), n, &total));
    if (total > 0x7FFFFFFFull)
        return fail(QEH_E_UNSUPPORTED, std::string(fname) + ": result larger than 2^31-1 bytes (Arrow Utf8 uses int32 offsets)");
    QEH_TRY(alloc_utf8(ctx, n, total, false, out));
    void *scr = nullptr;
    int s = scratch_zeroed(ctx, 64, &scr);
    if (s == QEH_OK) {
        const int64_t work = std::max<int64_t>((int64_t)((total + 15) >> 4), n + 1);
        KernelTimer kt(ctx, "str_rows");
        hipLaunchKernelGGL(k_str_rows_write, dim3(grid_for(ctx, work, kBlock, 8)), dim3(kBlock), 0, ctx->stream, ops, n,
                           excl.as<uint64_t>(), total, (uint8_t *)out->values, out->offsets, (uint32_t *)scr);
    }
    if (s == QEH_OK && hipGetLastError() != hipSuccess) s = fail(QEH_E_HIP, std::string(fname) + ": kernel launch failed");
    uint32_t flag = 0;
    if (s == QEH_OK) s = read_small(ctx, &flag, scr, 4);  // also orders len / excl's release after their readers
    if (s == QEH_OK && flag) s = non_ascii(fname);
    if (s != QEH_OK) {
        qeh_column_release(ctx, out);
        return s;
    }
    if (nullable) {
        out->validity = (uint8_t *)valid.release();
        out->null_count = -1;
    }
    return QEH_OK;
}

// One argument of a function after evaluation: a column, or a literal leaf.
struct FnArg {
    bool is_lit = false;
    qeh_expr_node lit{};
    qeh_column col{};
    int col_index = -1;  // a COLUMN leaf: its index in the rewrite's columns
    int type() const { return is_lit ? (lit.lit_is_null ? (int)QEH_DT_NULL : lit.lit_dtype) : col.dtype; }
};

int str_operand(qeh_ctx *ctx, const FnArg &a, FnRewrite *rw, StrOperand *o) {
    *o = StrOperand{};
    if (a.is_lit) {
        const int32_t len = a.lit.index;
        if (len < 0 || (len > 0 && a.lit.lit_i64 == 0)) return fail(QEH_E_INVALID, "Utf8 literal without bytes");
        rw->bufs.push_back(std::make_unique<DevBuf>());
        DevBuf &buf = *rw->bufs.back();
        QEH_TRY(buf.alloc(ctx, (size_t)std::max(len, 1)));
        if (len > 0)
            QEH_HIP(hipMemcpyAsync(buf.p, (const void *)(uintptr_t)a.lit.lit_i64, (size_t)len, hipMemcpyHostToDevice,
                                   ctx->stream));
        o->data = buf.as<uint8_t>();
        o->lit_len = len;
        o->is_lit = 1;
        return QEH_OK;
    }
    QEH_TRY(check_column(a.col, "scalar function argument"));
    if (a.col.length > 0 && !a.col.offsets) return fail(QEH_E_INVALID, "Utf8 column without offsets");
    o->offs = a.col.offsets + a.col.offset;
    o->data = (const uint8_t *)a.col.values;
    return QEH_OK;
}

// CONCAT of the operands; more than one pass holds are folded left to right (a CONCAT result has no
// NULLs and its slots are its strings, so CONCAT(CONCAT(a..h), i) = CONCAT(a..i)).
int str_concat(qeh_ctx *ctx, std::vector<FnArg> args, int64_t n, FnRewrite *rw, qeh_column *out) {
    for (;;) {
        StrOperands ops{};
        ops.mode = STR_CONCAT;
        ops.k = (int)std::min<size_t>(args.size(), kMaxStrOps);
        for (int j = 0; j < ops.k; ++j) QEH_TRY(str_operand(ctx, args[j], rw, &ops.op[j]));
        qeh_column r{};
        QEH_TRY(str_rows(ctx, ops, n, false, "CONCAT", &r));
        if ((size_t)ops.k == args.size()) {
            *out = r;
            return QEH_OK;
        }
        rw->args.push_back(r);
        FnArg folded;
        folded.col = r;
        args.erase(args.begin(), args.begin() + ops.k);
        args.insert(args.begin(), folded);
    }
}

}  // namespace

FnRewrite::~FnRewrite() {
    if (!ctx) return;
    if (!temps.empty() || !args.empty() || !bufs.empty()) (void)hipStreamSynchronize(ctx->stream);
    for (auto &c : temps) qeh_column_release(ctx, &c);
    for (auto &c : args) qeh_column_release(ctx, &c);
}

qeh_column FnRewrite::take(int ci) {
    qeh_column c = temps[ci - n_in];
    temps[ci - n_in].owned = 0;
    return c;
}

// The function `fn` over its evaluated arguments -> *node, the leaf that replaces its subtree.
static int apply_function(qeh_ctx *ctx, const qeh_expr_node &fn, std::vector<FnArg> &args, int64_t n, FnRewrite *rw,
                          qeh_expr_node *node) {
    std::vector<int> types;
    for (auto &a : args) types.push_back(a.type());
    int rt = 0;
    QEH_TRY(scalar_fn_type(fn.op, types.data(), (int)types.size(), &rt));
    // a literal where a kernel reads a column: broadcast it (numbers through qeh_eval's literal
    // program, strings through one CONCAT pass)
    auto as_column = [&](FnArg &a) -> int {
        if (!a.is_lit) return QEH_OK;
        qeh_column c{};
        if (a.type() == QEH_DT_UTF8) {
            QEH_TRY(str_concat(ctx, {a}, n, rw, &c));
        } else {
            const qeh_expr one{&a.lit, 1};
            QEH_TRY(qeh_eval(ctx, nullptr, 0, &one, n, &c));
        }
        rw->args.push_back(c);
        a.is_lit = false;
        a.col = c;
        return QEH_OK;
    };
    qeh_column res{};
    switch (fn.op) {
        case QEH_FN_COALESCE:  // its first argument, unchanged (operators.rs:249-250)
            if (args[0].is_lit) {
                *node = args[0].lit;
                return QEH_OK;
            }
            if (args[0].col_index >= 0) {
                *node = qeh_expr_node{};
                node->kind = QEH_EX_COLUMN;
                node->index = args[0].col_index;
                return QEH_OK;
            }
            // an evaluated argument: it moves from the arguments to the appended columns
            for (size_t i = 0; i < rw->args.size(); ++i)
                if (rw->args[i].values == args[0].col.values && rw->args[i].offsets == args[0].col.offsets) {
                    res = rw->args[i];
                    rw->args.erase(rw->args.begin() + i);
                    break;
                }
            if (!res.values) return fail(QEH_E_INTERNAL, "COALESCE: argument column not found");
            break;
        case QEH_FN_UPPER: case QEH_FN_LOWER: {
            QEH_TRY(as_column(args[0]));
            const qeh_column &c = args[0].col;
            if (!has_nulls(c)) {
                QEH_TRY(check_column(c, scalar_fn_name(fn.op)));
                QEH_TRY(str_case_stream(ctx, fn.op, c, n, &res));
            } else {
                StrOperands ops{};
                ops.mode = fn.op == QEH_FN_UPPER ? STR_UPPER : STR_LOWER;
                ops.k = 1;
                QEH_TRY(str_operand(ctx, args[0], rw, &ops.op[0]));
                ops.valid = make_colref(c);
                QEH_TRY(str_rows(ctx, ops, n, true, scalar_fn_name(fn.op), &res));
            }
            break;
        }
        case QEH_FN_LENGTH:
            QEH_TRY(as_column(args[0]));
            QEH_TRY(str_length(ctx, args[0].col, n, &res));
            break;
        case QEH_FN_CONCAT: QEH_TRY(str_concat(ctx, args, n, rw, &res)); break;
        case QEH_FN_POWER:
            QEH_TRY(as_column(args[0]));
            QEH_TRY(as_column(args[1]));
            QEH_TRY(scalar_math(ctx, fn.op, args[0].col, &args[1].col, n, &res));
            break;
        default:  // ABS / CEIL / FLOOR / ROUND / SQRT
            QEH_TRY(as_column(args[0]));
            QEH_TRY(scalar_math(ctx, fn.op, args[0].col, nullptr, n, &res));
            break;
    }
    rw->temps.push_back(res);
    rw->cols.push_back(res);
    *node = qeh_expr_node{};
    node->kind = QEH_EX_COLUMN;
    node->index = (int32_t)rw->cols.size() - 1;
    return QEH_OK;
}

int rewrite_scalar_functions(qeh_ctx *ctx, const qeh_column *cols, int n_cols, int64_t n_rows, const qeh_expr *e,
                             FnRewrite *out) {
    out->ctx = ctx;
    out->cols.assign(cols, cols + n_cols);
    out->n_in = n_cols;
    out->nodes.clear();
    out->changed = false;
    if (!expr_has_function(e)) return QEH_OK;
    std::vector<int> start;  // start[m]: first node of the subtree whose root is output node m
    // full-text match: a TO_TSVECTOR / TO_TSQUERY directly under an @@ is peeled into the mode of
    // the leaf that replaces it (ts_mode[m], QEH_TS_PLAIN for every other node); the @@ node then
    // runs the match kernel over its two operands and becomes a BOOL COLUMN leaf
    std::vector<char> ts_operand;
    std::vector<int> ts_mode;
    (void)ts_match_operands(e, &ts_operand);
    // nodes [first, second) of the output so far, evaluated: a leaf as it is, anything else
    // through qeh_eval over the columns it reads only (one kernel sees at most kMaxCols)
    auto eval_span = [&](int first_node, int second, FnArg *arg) -> int {
        const qeh_expr_node *x = out->nodes.data() + first_node;
        const int len = second - first_node;
        if (len == 1 && x->kind == QEH_EX_LITERAL) {
            arg->is_lit = true;
            arg->lit = *x;
            return QEH_OK;
        }
        if (len == 1 && x->kind == QEH_EX_COLUMN) {
            if (x->index < 0 || x->index >= (int)out->cols.size())
                return fail(QEH_E_INVALID, "Column index " + std::to_string(x->index) + " out of bounds");
            arg->col = out->cols[x->index];
            arg->col_index = x->index;
            return QEH_OK;
        }
        std::vector<qeh_expr_node> sub(x, x + len);
        std::vector<qeh_column> used;
        std::vector<int> pos_of(out->cols.size(), -1);
        for (auto &y : sub) {
            if (y.kind != QEH_EX_COLUMN) continue;
            if (y.index < 0 || y.index >= (int)out->cols.size())
                return fail(QEH_E_INVALID, "Column index " + std::to_string(y.index) + " out of bounds");
            if (pos_of[y.index] < 0) {
                pos_of[y.index] = (int)used.size();
                used.push_back(out->cols[y.index]);
            }
            y.index = pos_of[y.index];
        }
        const qeh_expr se{sub.data(), len};
        qeh_column r{};
        QEH_TRY(qeh_eval(ctx, used.data(), (int)used.size(), &se, n_rows, &r));
        if (r.owned) out->args.push_back(r);
        arg->col = r;
        return QEH_OK;
    };
    // the subtree from node `pos` on becomes one leaf
    auto replace_by = [&](int pos, const qeh_expr_node &leaf, int mode) {
        out->nodes.resize(pos);
        start.resize(pos);
        ts_mode.resize(pos);
        out->nodes.push_back(leaf);
        start.push_back(pos);
        ts_mode.push_back(mode);
        out->changed = true;
    };
    // an appended column: it joins the temporaries (moved there when it was an evaluated argument)
    auto append_column = [&](const qeh_column &c) -> qeh_expr_node {
        for (size_t i = 0; i < out->args.size(); ++i)
            if (out->args[i].values == c.values && out->args[i].offsets == c.offsets) {
                out->args.erase(out->args.begin() + i);
                break;
            }
        out->temps.push_back(c);
        out->cols.push_back(c);
        qeh_expr_node leaf{};
        leaf.kind = QEH_EX_COLUMN;
        leaf.index = (int32_t)out->cols.size() - 1;
        return leaf;
    };
    for (int i = 0; i < e->n_nodes; ++i) {
        const qeh_expr_node &nd = e->nodes[i];
        const int m = (int)out->nodes.size();
        int first = m;
        if (nd.kind == QEH_EX_BINARY) {
            if (m < 2 || start[m - 1] < 1) return fail(QEH_E_INVALID, "malformed expression (binary)");
            first = start[start[m - 1] - 1];
            if (nd.op == QEH_OP_TSMATCH) {
                // both operands are evaluated first, the left one's error before the right one's
                // (operators.rs:382-383), then the two downcasts fail in that order (:571-583)
                const int rfirst = start[m - 1];
                FnArg side[2];
                QEH_TRY(eval_span(first, rfirst, &side[0]));
                QEH_TRY(eval_span(rfirst, m, &side[1]));
                if (side[0].type() != QEH_DT_UTF8) return fail(QEH_E_TYPE, "@@ left operand must be tsvector (string)");
                if (side[1].type() != QEH_DT_UTF8) return fail(QEH_E_TYPE, "@@ right operand must be tsquery (string)");
                TsSide ts[2];
                for (int k = 0; k < 2; ++k) {
                    const int root = k == 0 ? rfirst - 1 : m - 1;
                    ts[k].mode = ts_mode[root];
                    if (side[k].is_lit) {
                        ts[k].lit = (const uint8_t *)(uintptr_t)side[k].lit.lit_i64;
                        ts[k].lit_len = side[k].lit.index;
                    } else {
                        ts[k].col = &side[k].col;
                    }
                }
                qeh_column res{};
                QEH_TRY(ts_match(ctx, ts[0], ts[1], n_rows, &res));
                replace_by(first, append_column(res), QEH_TS_PLAIN);
                continue;
            }
        } else if (nd.kind == QEH_EX_UNARY || nd.kind == QEH_EX_IN_SUBQUERY) {
            if (m < 1) return fail(QEH_E_INVALID, "malformed expression (unary)");
            first = start[m - 1];
        } else if (nd.kind == QEH_EX_SCALAR_FUNCTION) {
            std::vector<std::pair<int, int>> span(std::max(nd.index, 0));  // argument a = nodes [first, second)
            int pos = m;
            for (int a = nd.index - 1; a >= 0; --a) {
                if (pos < 1) return fail(QEH_E_INVALID, "malformed expression (scalar function arguments)");
                span[a] = {start[pos - 1], pos};
                pos = start[pos - 1];
            }
            // every argument is evaluated first: its own error wins (operators.rs:70-72)
            std::vector<FnArg> args(span.size());
            for (size_t a = 0; a < span.size(); ++a) QEH_TRY(eval_span(span[a].first, span[a].second, &args[a]));
            if (ts_operand[i]) {
                // evaluated as part of the match: its argument stands for it, cut by the function's mode
                std::vector<int> types;
                for (auto &a : args) types.push_back(a.type());
                int rt = 0;
                QEH_TRY(ts_fn_type(nd.op, types.data(), (int)types.size(), &rt));
                const int mode = nd.op == QEH_FN_TO_TSVECTOR ? QEH_TS_TSVECTOR : QEH_TS_TSQUERY;
                if (args[0].is_lit) {
                    replace_by(pos, args[0].lit, mode);
                } else if (args[0].col_index >= 0) {
                    qeh_expr_node leaf{};
                    leaf.kind = QEH_EX_COLUMN;
                    leaf.index = args[0].col_index;
                    replace_by(pos, leaf, mode);
                } else {
                    replace_by(pos, append_column(args[0].col), mode);
                }
                continue;
            }
            qeh_expr_node leaf{};
            QEH_TRY(apply_function(ctx, nd, args, n_rows, out, &leaf));
            replace_by(pos, leaf, QEH_TS_PLAIN);
            continue;
        }
        out->nodes.push_back(nd);
        start.push_back(first);
        ts_mode.push_back(QEH_TS_PLAIN);
    }
    QEH_HIP(hipStreamSynchronize(ctx->stream));  // literal host bytes are the caller's
    out->expr.nodes = out->nodes.data();
    out->expr.n_nodes = (int32_t)out->nodes.size();
    return QEH_OK;
}

}  // namespace qeh
