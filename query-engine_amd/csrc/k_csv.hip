// CSV scan: the bytes of a CSV file to typed Arrow columns (qeh_scan_csv), the input side of
// CsvDataSource::scan (crates/query-storage/src/csv.rs:23-38) and of the pgwire server's load_csv
// (crates/query-pgwire/src/server.rs:127-172), which both go through arrow-csv.  arrow-csv is not
// restated: the reader accepts the strict dialect of DESIGN.md §4 "CSV scan", is exact on it, and
// answers QEH_E_UNSUPPORTED (data row, column, reason) for everything else, so that the caller's
// host reader parses the file or raises its own error.
//
// Structure pass (threads own `chunk` consecutive bytes, a kernel argument):
//   k_csv_chunks   per chunk: its quotes, and the records that start in it counted twice -- for an
//                  even and for an odd number of quotes before the chunk
//   (scan of the quotes) k_csv_pick keeps the count of the chunk's true parity (scan of the counts)
//   k_csv_starts   the same walk with the parity known: record start offsets, int64, in file order
// A byte is inside quotes iff the number of quotes before it is odd; a record starts after a
// terminator at even parity, and records without bytes are skipped.  That equals the dialect's
// sequential parse up to the first quoting violation, which is all the field pass needs:
// Field pass (one thread per data row, the header rides with row 0):
//   k_csv_fields   walks its record with the dialect's sequential rules -- so it meets the first
//                  violation of the file in the right record and field, whatever the parity parse made
//                  of the bytes behind it -- checks UTF-8, the field count and each cell's grammar,
//                  writes the fixed-width values, one validity word per wave and column by ballot,
//                  the Utf8 lengths, and the rows whose double it cannot decide (parse_float.h)
//   (scan of the lengths per Utf8 column) k_csv_utf8 copies the strings, "" collapsed
// The first refusal is one 64-bit word (record, column, reason) reduced with atomicMin.
#include <algorithm>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "device_common.h"
#include "ops.h"
#include "parse_float.h"

namespace qeh {

constexpr int kCsvMaxCols = 32;
constexpr int kCsvChunkDefault = 64;

enum CsvReason {
    kCsvStrayQuote = 1, kCsvAfterQuote, kCsvUnterminated, kCsvTooFew, kCsvTooMany, kCsvUtf8, kCsvInt, kCsvFloat,
    kCsvBool, kCsvDate
};

const char *csv_reason_text(int r) {
    switch (r) {
        case kCsvStrayQuote: return "a quote inside an unquoted field";
        case kCsvAfterQuote: return "a byte other than a delimiter or terminator after a closing quote";
        case kCsvUnterminated: return "an unterminated quoted field";
        case kCsvTooFew: return "too few fields";
        case kCsvTooMany: return "too many fields";
        case kCsvUtf8: return "invalid UTF-8";
        case kCsvInt: return "not an integer of the column's type";
        case kCsvFloat: return "not a Float64";
        case kCsvBool: return "not a Boolean";
        case kCsvDate: return "not a Date32 (YYYY-MM-DD, years 0001-9999)";
        default: return "refused";
    }
}

struct CsvCol {
    int32_t dtype;
    int32_t _pad;
    void *values;           // fixed width: the value buffer (BOOL: bit-packed); Utf8: the byte buffer
    uint64_t *validity;     // one word per 64 rows
    uint32_t *len;          // Utf8: byte length per row
    const uint64_t *at;     // Utf8: exclusive scan of len
    int32_t *offsets;       // Utf8: Arrow offsets
    uint32_t *und_row;      // Float64: rows the device could not decide ...
    uint64_t *und_at;       // ... and their cell: byte offset | length << 40
};
struct CsvCols {
    CsvCol c[kCsvMaxCols];
    int32_t n;
};

// status words of one call
constexpr int kCsvWordErr = 0, kCsvWordNulls = 1, kCsvWordUnd = 1 + kCsvMaxCols, kCsvWords = 1 + 2 * kCsvMaxCols;

__device__ __forceinline__ bool csv_term(uint8_t c) { return c == '\n' || c == '\r'; }

// f(offset, byte) over bytes [lo, hi): single bytes up to the first 16-B aligned address, 16-B loads
// over the body, single bytes for the rest
template <class F>
__device__ __forceinline__ void csv_for_bytes(const uint8_t *p, int64_t lo, int64_t hi, F f) {
    int64_t i = lo;
    for (; i < hi && (((uintptr_t)(p + i)) & 15) != 0; ++i) f(i, p[i]);
    for (; i + 16 <= hi; i += 16) {
        const uint4 v = *reinterpret_cast<const uint4 *>(p + i);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 16; ++k) f(i + k, (uint8_t)(w[k >> 2] >> ((k & 3) * 8)));
    }
    for (; i < hi; ++i) f(i, p[i]);
}

// The records that start in chunk t.  A record starts at s when the quotes before s are even, s is
// the first byte of the input or follows a terminator, and s is no terminator itself (an empty
// record; the "\n" of "\r\n").  WRITE = false: *quotes = the chunk's quotes, *cnt = starts for an
// even parity before the chunk | starts for an odd one << 16.  WRITE = true: `odd` = that parity,
// the starts go to starts[base ..].
template <bool WRITE>
__device__ __forceinline__ void csv_walk_chunk(const uint8_t *p, int64_t size, int64_t t, int chunk, bool odd, uint32_t *quotes,
                                               uint32_t *cnt, int64_t *starts, uint64_t base) {
    const int64_t lo = t * chunk, hi = lo + chunk < size ? lo + chunk : size;
    bool prev_term = lo == 0 || csv_term(p[lo - 1]);
    uint32_t q = 0, n_even = 0, n_odd = 0;
    csv_for_bytes(p, lo, hi, [&](int64_t i, uint8_t c) {
        const bool term = csv_term(c);
        if (prev_term && !term) {
            const bool inside = ((q & 1u) != 0) != odd;
            if (WRITE) {
                if (!inside) starts[base + n_even] = i;
                n_even += !inside;
            } else {
                n_even += !inside;
                n_odd += inside;
            }
        }
        q += c == '"';
        prev_term = term;
    });
    if (!WRITE) {
        *quotes = q;
        *cnt = n_even | (n_odd << 16);
    }
}

__global__ __launch_bounds__(kBlock) void k_csv_chunks(const uint8_t *__restrict__ p, int64_t size, int chunk, int64_t n_chunks,
                                                      uint32_t *__restrict__ quotes, uint32_t *__restrict__ cnt) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_chunks) return;
    csv_walk_chunk<false>(p, size, t, chunk, false, quotes + t, cnt + t, nullptr, 0);
}

// quotes[t] := the parity before chunk t, cnt[t] := the record starts of that parity
__global__ __launch_bounds__(kBlock) void k_csv_pick(const uint64_t *__restrict__ qoff, int64_t n_chunks, uint32_t *__restrict__ quotes,
                                                    uint32_t *__restrict__ cnt) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_chunks) return;
    const uint32_t odd = (uint32_t)(qoff[t] & 1u), c = cnt[t];
    quotes[t] = odd;
    cnt[t] = odd ? c >> 16 : c & 0xFFFFu;
}

__global__ __launch_bounds__(kBlock) void k_csv_starts(const uint8_t *__restrict__ p, int64_t size, int chunk, int64_t n_chunks,
                                                      const uint32_t *__restrict__ parity, const uint64_t *__restrict__ roff,
                                                      int64_t *__restrict__ starts) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= n_chunks) return;
    csv_walk_chunk<true>(p, size, t, chunk, parity[t] != 0, nullptr, nullptr, starts, roff[t]);
}

// The input through a one-word cache: 8-B loads where the whole word lies inside the buffer, single
// bytes at its two ends.
struct CsvBytes {
    const uint8_t *p;
    int64_t size;
    uintptr_t cur = ~(uintptr_t)0;
    uint64_t w = 0;
    __device__ __forceinline__ uint8_t at(int64_t i) {
        const uintptr_t a = (uintptr_t)p + (uintptr_t)i, wa = a & ~(uintptr_t)7;
        if (wa != cur) {
            if (wa >= (uintptr_t)p && wa + 8 <= (uintptr_t)p + (uintptr_t)size) {
                w = *reinterpret_cast<const uint64_t *>(wa);
            } else {
                w = 0;
                for (int k = 0; k < 8; ++k) {
                    const uintptr_t b = wa + k;
                    if (b >= (uintptr_t)p && b < (uintptr_t)p + (uintptr_t)size)
                        w |= (uint64_t)(*reinterpret_cast<const uint8_t *>(b)) << (8 * k);
                }
            }
            cur = wa;
        }
        return (uint8_t)(w >> ((a & 7) * 8));
    }
};

// One field by the dialect's sequential rules.  pos: its first byte (== size: the empty field after
// a delimiter that ends the input).  Content = bytes [a, b) with `esc` "" pairs inside; the next
// field starts at *next unless *ended (terminator or end of input).  Returns 0 or a CsvReason.
struct CsvField {
    int64_t a, b, next;
    uint32_t esc;
    bool ended;
};
// UTF-8 by its well-formed byte ranges (Unicode 15 table 3-7): `need` continuation bytes are due,
// the next one within [lo, hi]
struct CsvUtf8 {
    uint32_t need = 0, lo = 0x80, hi = 0xBF;
    __device__ __forceinline__ bool step(uint8_t c) {
        if (need) {
            if (c < lo || c > hi) return false;
            --need, lo = 0x80, hi = 0xBF;
            return true;
        }
        if (c < 0x80) return true;
        if (c >= 0xC2 && c <= 0xDF) need = 1;
        else if (c >= 0xE0 && c <= 0xEF) need = 2, lo = c == 0xE0 ? 0xA0 : 0x80, hi = c == 0xED ? 0x9F : 0xBF;
        else if (c >= 0xF0 && c <= 0xF4) need = 3, lo = c == 0xF0 ? 0x90 : 0x80, hi = c == 0xF4 ? 0x8F : 0xBF;
        else return false;
        return true;
    }
};

template <bool CHECK>
__device__ __forceinline__ int csv_scan_field(CsvBytes &s, int64_t pos, CsvField *f) {
    const int64_t size = s.size;
    CsvUtf8 u;
    f->esc = 0;
    f->ended = false;
    f->next = size;
    int64_t i = pos;
    if (pos < size && s.at(pos) == '"') {
        f->a = ++i;
        for (;;) {
            if (i >= size) return kCsvUnterminated;
            const uint8_t c = s.at(i);
            if (CHECK && !u.step(c)) return kCsvUtf8;
            if (c == '"') {
                if (i + 1 < size && s.at(i + 1) == '"') {
                    ++f->esc;
                    i += 2;
                    continue;
                }
                break;
            }
            ++i;
        }
        f->b = i++;
        if (i >= size) f->ended = true;
        else {
            const uint8_t c = s.at(i);
            if (c == ',') f->next = i + 1;
            else if (csv_term(c)) f->ended = true;
            else return kCsvAfterQuote;
        }
        return 0;
    }
    f->a = pos;
    for (;; ++i) {
        if (i >= size) {
            if (CHECK && u.need) return kCsvUtf8;
            f->b = i;
            f->ended = true;
            return 0;
        }
        const uint8_t c = s.at(i);
        if (CHECK && !u.step(c)) return kCsvUtf8;
        if (c == ',') {
            f->b = i;
            f->next = i + 1;
            return 0;
        }
        if (csv_term(c)) {
            f->b = i;
            f->ended = true;
            return 0;
        }
        if (CHECK && c == '"') return kCsvStrayQuote;
    }
}

__device__ __forceinline__ void csv_refuse(uint64_t *status, int64_t rec, int col, int reason) {
    atomicMin((unsigned long long *)(status + kCsvWordErr),
              ((unsigned long long)rec << 24) | ((unsigned long long)col << 8) | (unsigned long long)reason);
}

// the header (record 0 when has_header): only its fields are counted
__device__ void csv_check_header(CsvBytes &s, int64_t pos, int n_cols, uint64_t *status) {
    CsvField f;
    for (int c = 0;; ++c) {
        if (c == n_cols) return csv_refuse(status, 0, n_cols, kCsvTooMany);
        const int r = csv_scan_field<true>(s, pos, &f);
        if (r) return csv_refuse(status, 0, c, r);
        if (f.ended) {
            if (c + 1 < n_cols) csv_refuse(status, 0, c + 1, kCsvTooFew);
            return;
        }
        pos = f.next;
    }
}

// Thread i = data row i = record i + has_header; a wave holds 64 consecutive rows, so the validity
// word (and a BOOL column's value word) of those rows is one ballot.  The grid covers max(n_rows, 1)
// threads: thread 0 also checks the header.
__global__ __launch_bounds__(kBlock) void k_csv_fields(const uint8_t *__restrict__ p, int64_t size, const int64_t *__restrict__ starts,
                                                      int64_t n_rows, int has_header, CsvCols cols, uint64_t *__restrict__ status) {
    const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool active = row < n_rows;
    const int64_t rec = row + has_header;
    CsvBytes s{p, size};
    if (row == 0 && has_header) csv_check_header(s, starts[0], cols.n, status);
    int64_t pos = active ? starts[rec] : 0;
    bool dead = !active, ended = false;
    const int64_t word = row >> 6;
    const bool wave_has_rows = (row & ~(int64_t)63) < n_rows;
    for (int c = 0; c < cols.n; ++c) {
        const CsvCol &col = cols.c[c];
        bool valid = false, bit = false;
        uint64_t v = 0;
        uint32_t len = 0;
        if (!dead) {
            CsvField f;
            int r = ended ? (int)kCsvTooFew : csv_scan_field<true>(s, pos, &f);
            if (!r) {
                ended = f.ended;
                pos = f.next;
                const int64_t n = f.b - f.a - (int64_t)f.esc;
                valid = n > 0;
                if (valid) {
                    if (col.dtype == QEH_DT_UTF8) {
                        if (n > 0x7FFFFFFF) len = 0x80000000u;  // (the column total then exceeds the Arrow limit)
                        else len = (uint32_t)n;
                    } else if (f.esc) {
                        r = col.dtype == QEH_DT_FLOAT64 ? kCsvFloat : col.dtype == QEH_DT_BOOL ? kCsvBool
                            : col.dtype == QEH_DT_DATE32 ? kCsvDate : kCsvInt;
                    } else {
                        switch (col.dtype) {
                            case QEH_DT_INT32: case QEH_DT_INT64: {
                                int64_t x = 0;
                                if (parse_int_text(s, f.a, f.b, col.dtype == QEH_DT_INT32 ? 0x7FFFFFFFull : 0x7FFFFFFFFFFFFFFFull, &x))
                                    r = kCsvInt;
                                v = (uint64_t)x;
                                break;
                            }
                            case QEH_DT_FLOAT64: {
                                const int pr = parse_f64_text(s, f.a, f.b, &v);
                                if (pr == kParseBad) r = kCsvFloat;
                                else if (pr == kParseUndecided) {
                                    const uint32_t slot = (uint32_t)atomicAdd((unsigned long long *)(status + kCsvWordUnd + c), 1ull);
                                    col.und_row[slot] = (uint32_t)row;
                                    col.und_at[slot] = (uint64_t)f.a | ((uint64_t)(f.b - f.a) << 40);
                                    v = 0;
                                }
                                break;
                            }
                            case QEH_DT_BOOL:
                                if (parse_bool_text(s, f.a, f.b, &bit)) r = kCsvBool;
                                break;
                            default: {  // QEH_DT_DATE32
                                int32_t d = 0;
                                if (parse_date32_text(s, f.a, f.b, &d)) r = kCsvDate;
                                v = (uint64_t)(int64_t)d;
                                break;
                            }
                        }
                    }
                }
            }
            if (r) {
                csv_refuse(status, rec, c, r);
                dead = true, valid = false, bit = false, v = 0, len = 0;
            }
        }
        if (active) {
            switch (col.dtype) {
                case QEH_DT_INT32: case QEH_DT_DATE32: ((int32_t *)col.values)[row] = (int32_t)v; break;
                case QEH_DT_INT64: case QEH_DT_FLOAT64: ((uint64_t *)col.values)[row] = v; break;
                case QEH_DT_UTF8: col.len[row] = len; break;
                default: break;
            }
        }
        const uint64_t vmask = __ballot(valid), amask = __ballot(active);
        const uint64_t bmask = col.dtype == QEH_DT_BOOL ? __ballot(bit) : 0;
        if ((threadIdx.x & 63) == 0 && wave_has_rows) {
            col.validity[word] = vmask;
            if (col.dtype == QEH_DT_BOOL) ((uint64_t *)col.values)[word] = bmask;
            const unsigned nulls = popc64(amask & ~vmask);
            if (nulls) atomicAdd((unsigned long long *)(status + kCsvWordNulls + c), (unsigned long long)nulls);
        }
    }
    if (!dead && !ended) csv_refuse(status, rec, cols.n, kCsvTooMany);
}

// The Utf8 columns of a table that passed k_csv_fields: offsets and bytes, "" written as one quote.
__global__ __launch_bounds__(kBlock) void k_csv_utf8(const uint8_t *__restrict__ p, int64_t size, const int64_t *__restrict__ starts,
                                                    int64_t n_rows, int has_header, CsvCols cols) {
    const int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (row >= n_rows) return;
    CsvBytes s{p, size};
    int64_t pos = starts[row + has_header];
    for (int c = 0; c < cols.n; ++c) {
        const CsvCol &col = cols.c[c];
        CsvField f;
        if (csv_scan_field<false>(s, pos, &f)) return;  // (cannot happen after the check pass)
        pos = f.next;
        if (col.dtype != QEH_DT_UTF8) continue;
        const uint64_t at = col.at[row];
        col.offsets[row] = (int32_t)at;
        if (row == n_rows - 1) col.offsets[n_rows] = (int32_t)(at + col.len[row]);
        uint8_t *o = (uint8_t *)col.values + at;
        if (!f.esc) {
            for (int64_t i = f.a; i < f.b; ++i) *o++ = s.at(i);
        } else {
            for (int64_t i = f.a; i < f.b; ++i) {
                const uint8_t ch = s.at(i);
                *o++ = ch;
                if (ch == '"') ++i;  // the pair's second quote
            }
        }
    }
}

__global__ void k_csv_patch(double *__restrict__ values, const uint32_t *__restrict__ rows, const double *__restrict__ v, int64_t n) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) values[rows[i]] = v[i];
}

namespace {

int csv_chunk_bytes() {
    const char *e = std::getenv("QEH_CSV_CHUNK");  // test geometry, read per call
    if (!e) return kCsvChunkDefault;
    const int v = std::atoi(e);
    return v >= 1 && v <= 32768 ? v : kCsvChunkDefault;
}

struct CsvOut {  // releases what the call allocated unless it succeeds
    qeh_ctx *ctx;
    std::vector<qeh_column> cols;
    ~CsvOut() {
        for (qeh_column &c : cols)
            if (c.owned) qeh_column_release(ctx, &c);
    }
};

// rows the device left undecided: strtod on the host (glibc rounds correctly), one scatter back
int csv_patch_floats(qeh_ctx *ctx, const uint8_t *host_bytes, const uint8_t *dev_bytes, const CsvCol &col, uint64_t n) {
    std::vector<uint32_t> rows(n);
    std::vector<uint64_t> at(n);
    std::vector<double> vals(n);
    QEH_HIP(hipMemcpyAsync(rows.data(), col.und_row, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    QEH_HIP(hipMemcpyAsync(at.data(), col.und_at, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    QEH_HIP(hipStreamSynchronize(ctx->stream));
    std::string cell;
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t off = at[i] & ((1ull << 40) - 1), len = at[i] >> 40;
        cell.resize(len);
        if (host_bytes) std::memcpy(&cell[0], host_bytes + off, len);
        else {
            QEH_HIP(hipMemcpyAsync(&cell[0], dev_bytes + off, len, hipMemcpyDeviceToHost, ctx->stream));
            QEH_HIP(hipStreamSynchronize(ctx->stream));
        }
        vals[i] = std::strtod(cell.c_str(), nullptr);
    }
    DevBuf drows, dvals;
    QEH_TRY(drows.alloc(ctx, n * 4));
    QEH_TRY(dvals.alloc(ctx, n * 8));
    QEH_HIP(hipMemcpyAsync(drows.p, rows.data(), n * 4, hipMemcpyHostToDevice, ctx->stream));
    QEH_HIP(hipMemcpyAsync(dvals.p, vals.data(), n * 8, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(k_csv_patch, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream,
                       (double *)col.values, drows.as<uint32_t>(), dvals.as<double>(), (int64_t)n);
    QEH_HIP(hipGetLastError());
    QEH_HIP(hipStreamSynchronize(ctx->stream));  // the host vectors die here
    return QEH_OK;
}

}  // namespace

int scan_csv(qeh_ctx *ctx, const uint8_t *bytes, int64_t size, int bytes_on_device, int has_header, const int32_t *dtypes,
             int n_cols, qeh_column *out_cols, int64_t *out_rows) {
    if (!ctx || size < 0 || (size > 0 && !bytes) || !dtypes || n_cols < 1 || !out_cols || !out_rows ||
        (has_header != 0 && has_header != 1))
        return fail(QEH_E_INVALID, "qeh_scan_csv: bad argument");
    for (int c = 0; c < n_cols; ++c) {
        switch (dtypes[c]) {
            case QEH_DT_BOOL: case QEH_DT_INT32: case QEH_DT_INT64: case QEH_DT_FLOAT64: case QEH_DT_UTF8: case QEH_DT_DATE32:
                break;
            case QEH_DT_FLOAT32: case QEH_DT_DATE64: case QEH_DT_TIMESTAMP_S: case QEH_DT_TIMESTAMP_MS: case QEH_DT_TIMESTAMP_US:
            case QEH_DT_TIMESTAMP_NS:
                return fail(QEH_E_UNSUPPORTED, "csv: schema, column " + std::to_string(c) + ": " + arrow_type_name(dtypes[c]) +
                                                   " cells are not read on the device");
            default: return fail(QEH_E_INVALID, "qeh_scan_csv: column " + std::to_string(c) + " has no readable dtype");
        }
    }
    if (n_cols > kCsvMaxCols) return fail(QEH_E_UNSUPPORTED, "csv: schema: at most 32 columns per call");
    if (size >= (int64_t(1) << 40)) return fail(QEH_E_UNSUPPORTED, "csv: input of 1 TiB or more");
    DeviceGuard dg(ctx->device);

    DevBuf upload;
    const uint8_t *host_bytes = bytes_on_device ? nullptr : bytes;
    const uint8_t *p = bytes;
    if (!bytes_on_device) {
        QEH_TRY(upload.alloc(ctx, (size_t)std::max<int64_t>(size, 8)));
        if (size) QEH_HIP(hipMemcpyAsync(upload.p, bytes, (size_t)size, hipMemcpyHostToDevice, ctx->stream));
        p = upload.as<uint8_t>();
    }

    // ---- structure pass: record starts
    const int chunk = csv_chunk_bytes();
    const int64_t n_chunks = (size + chunk - 1) / chunk;
    uint64_t n_rec = 0;
    DevBuf quotes, cnt, off, starts;
    if (n_chunks > 0) {
        if (n_chunks > 0x7FFFFFFFll * kBlock) return fail(QEH_E_UNSUPPORTED, "csv: input too large for the chunk size");
        const unsigned grid = (unsigned)((n_chunks + kBlock - 1) / kBlock);
        QEH_TRY(quotes.alloc(ctx, (size_t)n_chunks * 4));
        QEH_TRY(cnt.alloc(ctx, (size_t)n_chunks * 4));
        QEH_TRY(off.alloc(ctx, (size_t)n_chunks * 8));
        {
            KernelTimer kt(ctx, "csv_chunks");
            hipLaunchKernelGGL(k_csv_chunks, dim3(grid), dim3(kBlock), 0, ctx->stream, p, size, chunk, n_chunks, quotes.as<uint32_t>(),
                               cnt.as<uint32_t>());
        }
        QEH_HIP(hipGetLastError());
        DevBuf tot;
        QEH_TRY(tot.alloc(ctx, 8));
        QEH_TRY(exclusive_scan_u32_dev(ctx, quotes.as<uint32_t>(), off.as<uint64_t>(), n_chunks, tot.as<uint64_t>()));
        {
            KernelTimer kt(ctx, "csv_pick");
            hipLaunchKernelGGL(k_csv_pick, dim3(grid), dim3(kBlock), 0, ctx->stream, off.as<uint64_t>(), n_chunks, quotes.as<uint32_t>(),
                               cnt.as<uint32_t>());
        }
        QEH_HIP(hipGetLastError());
        QEH_TRY(exclusive_scan_u32(ctx, cnt.as<uint32_t>(), off.as<uint64_t>(), n_chunks, &n_rec));
        if (n_rec >= 0x7FFFFFFFull) return fail(QEH_E_UNSUPPORTED, "csv: 2^31 - 1 records or more");
        QEH_TRY(starts.alloc(ctx, (size_t)std::max<uint64_t>(n_rec, 1) * 8));
        if (n_rec > 0) {
            KernelTimer kt(ctx, "csv_starts");
            hipLaunchKernelGGL(k_csv_starts, dim3(grid), dim3(kBlock), 0, ctx->stream, p, size, chunk, n_chunks, quotes.as<uint32_t>(),
                               off.as<uint64_t>(), starts.as<int64_t>());
        }
        QEH_HIP(hipGetLastError());
        quotes.reset(), cnt.reset(), off.reset();
    }
    const int hdr = has_header && n_rec > 0 ? 1 : 0;
    const int64_t n_rows = (int64_t)n_rec - hdr;

    // ---- field pass
    CsvOut out{ctx, std::vector<qeh_column>((size_t)n_cols)};
    for (qeh_column &c : out.cols) std::memset(&c, 0, sizeof(c));
    CsvCols cc{};
    cc.n = n_cols;
    std::vector<DevBuf> len((size_t)n_cols), at((size_t)n_cols), und_row((size_t)n_cols), und_at((size_t)n_cols);
    const size_t vbytes = std::max<size_t>((size_t)((n_rows + 63) / 64) * 8, 8);
    for (int c = 0; c < n_cols; ++c) {
        qeh_column &o = out.cols[(size_t)c];
        cc.c[c].dtype = dtypes[c];
        if (dtypes[c] == QEH_DT_UTF8) {
            o.dtype = QEH_DT_UTF8, o.owned = 1, o.length = n_rows;
            void *v = nullptr;
            QEH_TRY(ctx->pool->alloc(vbytes, &v));
            o.validity = (uint8_t *)v;
            QEH_TRY(len[(size_t)c].alloc(ctx, (size_t)std::max<int64_t>(n_rows, 1) * 4));
            cc.c[c].len = len[(size_t)c].as<uint32_t>();
        } else {
            QEH_TRY(alloc_column(ctx, dtypes[c], n_rows, true, &o));
            cc.c[c].values = o.values;
            if (dtypes[c] == QEH_DT_FLOAT64) {
                QEH_TRY(und_row[(size_t)c].alloc(ctx, (size_t)std::max<int64_t>(n_rows, 1) * 4));
                QEH_TRY(und_at[(size_t)c].alloc(ctx, (size_t)std::max<int64_t>(n_rows, 1) * 8));
                cc.c[c].und_row = und_row[(size_t)c].as<uint32_t>();
                cc.c[c].und_at = und_at[(size_t)c].as<uint64_t>();
            }
        }
        cc.c[c].validity = (uint64_t *)o.validity;
    }
    uint64_t st[kCsvWords];
    std::memset(st, 0, sizeof(st));
    st[kCsvWordErr] = ~0ull;
    if (n_rec > 0) {
        DevBuf status;
        QEH_TRY(status.alloc(ctx, sizeof(st)));
        QEH_HIP(hipMemsetAsync(status.p, 0, sizeof(st), ctx->stream));
        QEH_HIP(hipMemsetAsync(status.p, 0xFF, 8, ctx->stream));
        {
            KernelTimer kt(ctx, "csv_fields");
            const unsigned grid = (unsigned)((std::max<int64_t>(n_rows, 1) + kBlock - 1) / kBlock);
            hipLaunchKernelGGL(k_csv_fields, dim3(grid), dim3(kBlock), 0, ctx->stream, p, size, starts.as<int64_t>(), n_rows, hdr, cc,
                               status.as<uint64_t>());
        }
        QEH_HIP(hipGetLastError());
        QEH_TRY(read_small(ctx, st, status.p, sizeof(st)));
    }
    if (st[kCsvWordErr] != ~0ull) {
        const int64_t rec = (int64_t)(st[kCsvWordErr] >> 24);
        const int col = (int)((st[kCsvWordErr] >> 8) & 0xFFFF), reason = (int)(st[kCsvWordErr] & 0xFF);
        return fail(QEH_E_UNSUPPORTED, "csv: row " + std::to_string(rec - hdr) + ", column " + std::to_string(col) + ": " +
                                           csv_reason_text(reason));
    }
    int64_t patched = 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (int c = 0; c < n_cols; ++c) {
        const uint64_t n = st[kCsvWordUnd + c];
        if (dtypes[c] == QEH_DT_FLOAT64 && n > 0) {
            QEH_TRY(csv_patch_floats(ctx, host_bytes, p, cc.c[c], n));
            patched += (int64_t)n;
        }
    }
    if (ctx->timing && patched) {  // qeh_kernel_time("csv_float_patch"): host milliseconds, cells parsed on the host
        auto &slot = ctx->timing_done["csv_float_patch"];
        slot.first += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        slot.second += patched;
    }
    bool any_utf8 = false;
    for (int c = 0; c < n_cols; ++c) {
        if (dtypes[c] != QEH_DT_UTF8) continue;
        any_utf8 = true;
        qeh_column &o = out.cols[(size_t)c];
        uint64_t total = 0;
        QEH_TRY(at[(size_t)c].alloc(ctx, (size_t)std::max<int64_t>(n_rows, 1) * 8));
        QEH_TRY(exclusive_scan_u32(ctx, cc.c[c].len, at[(size_t)c].as<uint64_t>(), n_rows, &total));
        if (total > 0x7FFFFFFFull)
            return fail(QEH_E_UNSUPPORTED, "csv: schema, column " + std::to_string(c) + ": a Utf8 column beyond 2^31 - 1 bytes");
        void *d = nullptr, *ofs = nullptr;
        QEH_TRY(ctx->pool->alloc(std::max<size_t>((size_t)total, 8), &d));
        o.values = d;
        o.values_bytes = (int64_t)total;
        QEH_TRY(ctx->pool->alloc((size_t)(n_rows + 1) * 4, &ofs));
        o.offsets = (int32_t *)ofs;
        if (n_rows == 0) QEH_HIP(hipMemsetAsync(ofs, 0, 4, ctx->stream));
        cc.c[c].values = d, cc.c[c].offsets = o.offsets, cc.c[c].at = at[(size_t)c].as<uint64_t>();
    }
    if (any_utf8 && n_rows > 0) {
        KernelTimer kt(ctx, "csv_utf8");
        hipLaunchKernelGGL(k_csv_utf8, dim3((unsigned)((n_rows + kBlock - 1) / kBlock)), dim3(kBlock), 0, ctx->stream, p, size,
                           starts.as<int64_t>(), n_rows, hdr, cc);
    }
    QEH_HIP(hipGetLastError());
    QEH_HIP(hipStreamSynchronize(ctx->stream));
    for (int c = 0; c < n_cols; ++c) {
        qeh_column &o = out.cols[(size_t)c];
        o.null_count = (int64_t)st[kCsvWordNulls + c];
        if (o.null_count == 0) {
            ctx->pool->free(o.validity);
            o.validity = nullptr;
        }
        out_cols[c] = o;
        o.owned = 0;  // handed over
    }
    *out_rows = n_rows;
    return QEH_OK;
}

}  // namespace qeh

extern "C" int qeh_scan_csv(qeh_ctx *ctx, const uint8_t *bytes, int64_t size, int bytes_on_device, int has_header,
                            const int32_t *dtypes, int n_cols, qeh_column *out_cols, int64_t *out_rows) {
    return qeh::scan_csv(ctx, bytes, size, bytes_on_device, has_header, dtypes, n_cols, out_cols, out_rows);
}
