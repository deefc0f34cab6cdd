// Full-text match: BinaryOp::TsMatch (`doc @@ query`) as evaluate_binary_op computes it
// (crates/query-executor/src/operators.rs:571-610) over operands that may be wrapped in TO_TSVECTOR /
// TO_TSQUERY (:261-318), without materialising a tsvector or tsquery string.
//
// A row is TRUE when every term of the query is one of the document's tokens, by byte equality.
// The pieces of a side follow its mode (enum qeh_ts_mode): white-space separated pieces as they
// are (a plain Utf8 expression), maximal [0-9A-Za-z] runs lower-cased (TO_TSVECTOR: the reference's
// sort and de-duplication do not change the set), or white-space separated pieces lower-cased
// (TO_TSQUERY).  The query's terms are its pieces without "&", "|" and pieces starting with '!'.
// White space is 0x09-0x0D and 0x20.  Only ASCII is mapped: a byte >= 0x80 in a non-NULL row sets a
// flag and the call returns QEH_E_UNSUPPORTED (Rust lower-cases and splits by Unicode rules).
//
// Kernels (each under its own KernelTimer name):
//   ts_match_stream  a literal query of <= kTsMaxTerms distinct terms (<= kTsTermBytes bytes), parsed
//                    once on the host into a term table staged in LDS.  A wave owns 64 consecutive
//                    rows and walks their concatenated bytes offsets[r0] .. offsets[r0 + 64] in steps
//                    of 1 KiB, one aligned 16-B load per lane, whatever the row lengths.  Per step a
//                    lane classifies its 16 bytes, token starts come from the token bits, the carry
//                    of the lane before (one ballot; the last lane's carries into the next step) and
//                    the row starts inside the chunk (the wave's 65 offsets sit in LDS); a lane that
//                    owns a token start looks its first byte up in the set of the terms' first bytes
//                    (two kernel arguments), and only then compares the token with the terms -- first byte,
//                    the token's end, the bytes -- and ORs the hits into its row's 64-bit mask in
//                    LDS.  After the range lane r tests row r's mask; values and validity leave as
//                    two ballots.
//   ts_match_rows    everything else (a query column, a literal document, more terms): one lane per
//                    row, the query's pieces against the document's pieces, each side folded by its
//                    own mode.  Always correct, not fast.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "device_common.h"
#include "ops.h"

namespace qeh {

constexpr int kTsMaxTerms = 64;      // one bit of a row's found-mask per term
constexpr int kTsTermBytes = 2048;   // LDS budget of the term bytes
constexpr int kTsWaves = kBlock / 64;
constexpr int kTsStep = 64 * 16;     // bytes a wave reads per step

__host__ __device__ __forceinline__ bool ts_space(uint32_t c) { return c == 0x20u || c - 9u < 5u; }
__host__ __device__ __forceinline__ bool ts_token_byte(int mode, uint32_t c) {
    if (mode == QEH_TS_TSVECTOR) return (c | 0x20u) - 'a' < 26u || c - '0' < 10u;
    return !ts_space(c);
}
__host__ __device__ __forceinline__ uint32_t ts_fold(int mode, uint32_t c) {
    return mode != QEH_TS_PLAIN && c - 'A' < 26u ? c + 32u : c;
}

// ---- (a) literal query: the stream kernel -----------------------------------------------------
// thdr[t] = offset of term t in tbytes | its length << 16; the terms are folded by the query's mode.
// first_lo / first_hi: the terms' first bytes (ASCII) as a 128-bit set, built by the host.
template <int MODE>
__global__ __launch_bounds__(kBlock) void k_ts_match_stream(const int32_t *__restrict__ offs, const uint8_t *__restrict__ data,
                                                            ColRef valid, int64_t n, const uint8_t *__restrict__ tbytes,
                                                            const uint32_t *__restrict__ thdr, int n_terms, int tbytes_len,
                                                            uint64_t first_lo, uint64_t first_hi,
                                                            uint64_t *__restrict__ out_bits,
                                                            uint64_t *__restrict__ out_valid, uint32_t *__restrict__ flag) {
    __shared__ uint8_t s_tb[kTsTermBytes];
    __shared__ uint32_t s_th[kTsMaxTerms];
    __shared__ int32_t s_off[kTsWaves][66];
    __shared__ unsigned long long s_mask[kTsWaves][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < tbytes_len; i += kBlock) s_tb[i] = tbytes[i];
    if (threadIdx.x < n_terms) s_th[threadIdx.x] = thdr[threadIdx.x];
    const unsigned long long full = n_terms >= 64 ? ~0ull : (1ull << n_terms) - 1;
    int32_t *off = s_off[wv];
    bool bad = false;  // a byte >= 0x80 in a valid row
    // every wave of a workgroup makes the same number of trips (the barriers), with no rows past n
    for (int64_t blk = blockIdx.x; blk * kBlock < n; blk += gridDim.x) {
        const int64_t w = blk * kTsWaves + wv, r0 = w * 64;
        const int nr = (int)(n - r0 < 0 ? 0 : (n - r0 < 64 ? n - r0 : 64));
        // the wave's offsets; entries past its rows repeat the last one (rows of no bytes)
        if (nr > 0) {
            off[lane] = offs[r0 + (lane < nr ? lane : nr)];
            if (lane == 0) off[64] = offs[r0 + nr];
        }
        s_mask[wv][lane] = 0;
        __syncthreads();
        const int64_t b0 = nr > 0 ? off[0] : 0, b1 = nr > 0 ? off[64] : 0;
        if (b1 > b0) {
            // steps start at the 16-B line of the first byte: an aligned line that holds one byte of
            // the column lies inside its allocation's pages
            const int64_t pos0 = b0 - (int64_t)(((uintptr_t)data + (uint64_t)b0) & 15);
            uint32_t carry = 0;  // the last byte of the step before was a token byte
            for (int64_t s = pos0; s < b1; s += kTsStep) {
                const int64_t cp = s + lane * 16;
                const bool live = cp < b1 && cp + 16 > b0;
                uint4 x = make_uint4(0, 0, 0, 0);
                if (live) x = *reinterpret_cast<const uint4 *>(data + cp);
                const int lo = (int)(b0 - cp > 0 ? b0 - cp : 0), hi = (int)(b1 - cp < 16 ? b1 - cp : 16);
                const uint32_t inr = live ? ((1u << hi) - 1) & ~((1u << lo) - 1) : 0;  // bytes of the range
                uint32_t tk = 0, hb = 0;
                const uint32_t xw[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const uint32_t c = (xw[j >> 2] >> (8 * (j & 3))) & 0xFFu;
                    tk |= (uint32_t)ts_token_byte(MODE, c) << j;
                    hb |= (c >> 7) << j;
                }
                tk &= inr;
                hb &= inr;
                const uint64_t last = __ballot((tk >> 15) & 1);
                const uint32_t prev = lane == 0 ? carry : (uint32_t)(last >> (lane - 1)) & 1u;
                carry = (uint32_t)(last >> 63);
                if (tk | hb) {
                    // the row of the chunk's first byte of the range: the last row starting at or before it
                    const int64_t p = cp + lo;
                    int row = 0, top = nr;
                    while (top - row > 1) {
                        const int mid = (row + top) >> 1;
                        if (off[mid] <= p) row = mid;
                        else top = mid;
                    }
                    // a row start always begins a token: tokens never join across rows
                    uint32_t rs = off[row] == p ? 1u << lo : 0;
                    for (int r = row + 1; r < nr; ++r) {  // these start after p
                        const int64_t o = off[r];
                        if (o >= cp + 16) break;
                        if (o > p) rs |= 1u << (int)(o - cp);
                    }
                    uint32_t ts = tk & (~((tk << 1) | prev) | rs);
                    int cur = row;
                    while (ts) {
                        const int j = __builtin_ctz(ts);
                        ts &= ts - 1;
                        const int64_t q = cp + j;
                        // most tokens end here: their first byte (still in registers) starts no term
                        const uint32_t wj = j < 8 ? (j < 4 ? x.x : x.y) : (j < 12 ? x.z : x.w);
                        const uint32_t c0 = ts_fold(MODE, (wj >> (8 * (j & 3))) & 0xFFu);
                        if (c0 >= 128u || !(((c0 < 64u ? first_lo : first_hi) >> (c0 & 63u)) & 1ull)) continue;
                        while (cur + 1 < nr && off[cur + 1] <= q) ++cur;
                        const int64_t rend = off[cur + 1] < b1 ? off[cur + 1] : b1;  // the token's row ends here
                        unsigned long long hit = 0;
                        for (int t = 0; t < n_terms; ++t) {
                            const uint32_t h = s_th[t];
                            const int to = (int)(h & 0xFFFFu), tl = (int)(h >> 16);
                            if (s_tb[to] != c0 || q + tl > rend) continue;
                            if (q + tl < rend && ts_token_byte(MODE, data[q + tl])) continue;  // the token goes on
                            // every byte of the candidate has to be a token byte of the document's mode:
                            // a term cut by another mode ('a&b' against a tsvector) spans separators
                            int k = 1;
                            for (; k < tl; ++k) {
                                const uint32_t c = data[q + k];
                                if (!ts_token_byte(MODE, c) || ts_fold(MODE, c) != s_tb[to + k]) break;
                            }
                            if (k == tl) hit |= 1ull << t;
                        }
                        if (hit) atomicOr(&s_mask[wv][cur], hit);
                    }
                    cur = row;
                    while (hb) {
                        const int j = __builtin_ctz(hb);
                        hb &= hb - 1;
                        while (cur + 1 < nr && off[cur + 1] <= cp + j) ++cur;
                        if (col_valid(valid, r0 + cur)) bad = true;
                    }
                }
            }
        }
        __syncthreads();
        const bool v = lane < nr && col_valid(valid, r0 + lane);
        const bool r = v && (s_mask[wv][lane] & full) == full;
        const uint64_t rb = __ballot(r), vb = __ballot(v);
        if (lane == 0 && nr > 0) {
            out_bits[w] = rb;
            if (out_valid) out_valid[w] = vb;
        }
        __syncthreads();  // the masks and offsets are rewritten by the next trip
    }
    if (__ballot(bad) != 0 && lane == 0) atomicOr(flag, 1u);
}

// ---- (b) the general form: one lane per row ------------------------------------------------------
struct TsOperand {
    ColRef valid;         // validity only (column side)
    const int32_t *offs;  // column side: offsets advanced by the column offset
    const uint8_t *data;  // column bytes, or the literal's bytes
    int32_t lit_len;
    int32_t is_lit;
    int32_t mode;
    int32_t _pad;
};

// The next piece of s[0, len) at or after *pos: [*st, *en); false when there is none.
__device__ __forceinline__ bool ts_next_piece(const uint8_t *s, int32_t len, int mode, int32_t *pos, int32_t *st, int32_t *en) {
    int32_t p = *pos;
    while (p < len && !ts_token_byte(mode, s[p])) ++p;
    if (p >= len) return false;
    *st = p;
    while (p < len && ts_token_byte(mode, s[p])) ++p;
    *en = *pos = p;
    return true;
}

__global__ __launch_bounds__(kBlock) void k_ts_match_rows(TsOperand d, TsOperand q, int64_t n, uint64_t *__restrict__ out_bits,
                                                          uint64_t *__restrict__ out_valid, uint32_t *__restrict__ flag) {
    const int lane = threadIdx.x & 63;
    const int64_t nw = (int64_t)gridDim.x * (blockDim.x / 64);
    uint32_t acc = 0;
    for (int64_t w = (int64_t)blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6); w * 64 < n; w += nw) {
        const int64_t i = w * 64 + lane;
        bool r = false, v = false;
        if (i < n) {
            const bool vd = d.is_lit || col_valid(d.valid, i), vq = q.is_lit || col_valid(q.valid, i);
            v = vd && vq;
            const uint8_t *pd = d.is_lit ? d.data : d.data + d.offs[i];
            const uint8_t *pq = q.is_lit ? q.data : q.data + q.offs[i];
            int32_t ld = d.is_lit ? d.lit_len : d.offs[i + 1] - d.offs[i];
            int32_t lq = q.is_lit ? q.lit_len : q.offs[i + 1] - q.offs[i];
            ld = ld > 0 ? ld : 0;
            lq = lq > 0 ? lq : 0;
            // non-ASCII: a non-NULL row of either side, whatever the other side's validity (the
            // host has looked at a literal)
            if (!d.is_lit && vd)
                for (int32_t k = 0; k < ld; ++k) acc |= pd[k];
            if (!q.is_lit && vq)
                for (int32_t k = 0; k < lq; ++k) acc |= pq[k];
            if (v) {
                r = true;
                int32_t qp = 0, ts = 0, te = 0;
                while (r && ts_next_piece(pq, lq, q.mode, &qp, &ts, &te)) {
                    const int32_t tl = te - ts;
                    const uint32_t c0 = pq[ts];
                    if (c0 == '!' || (tl == 1 && (c0 == '&' || c0 == '|'))) continue;  // not a term
                    bool found = false;
                    int32_t dp = 0, us = 0, ue = 0;
                    while (!found && ts_next_piece(pd, ld, d.mode, &dp, &us, &ue)) {
                        if (ue - us != tl) continue;
                        int32_t k = 0;
                        while (k < tl && ts_fold(d.mode, pd[us + k]) == ts_fold(q.mode, pq[ts + k])) ++k;
                        found = k == tl;
                    }
                    r = found;
                }
            }
        }
        const uint64_t rb = __ballot(r && v), vb = __ballot(v);
        if (lane == 0) {
            out_bits[w] = rb;
            if (out_valid) out_valid[w] = vb;
        }
    }
    if (__ballot((acc & 0x80u) != 0) != 0 && lane == 0) atomicOr(flag, 1u);
}

// ---- host --------------------------------------------------------------------------------------
namespace {

int ts_non_ascii() {
    return fail(QEH_E_UNSUPPORTED, "@@: non-ASCII input (a byte >= 0x80 in a non-NULL row or in a literal); the device "
                                   "tokenises ASCII only, the reference lower-cases and splits by Unicode rules");
}

// The distinct terms of a literal query under `mode`, folded: bytes and thdr as the stream kernel
// reads them.  false: more than it takes (the general kernel does).
bool ts_term_table(const uint8_t *s, int64_t len, int mode, std::vector<uint8_t> *bytes, std::vector<uint32_t> *hdr) {
    std::vector<std::string> terms;
    for (int64_t p = 0; p < len;) {
        while (p < len && !ts_token_byte(mode, s[p])) ++p;
        const int64_t st = p;
        while (p < len && ts_token_byte(mode, s[p])) ++p;
        if (p == st) break;
        std::string t((const char *)s + st, (size_t)(p - st));
        if (t[0] == '!' || t == "&" || t == "|") continue;
        for (auto &c : t) c = (char)ts_fold(mode, (uint8_t)c);
        if (std::find(terms.begin(), terms.end(), t) == terms.end()) terms.push_back(t);
        if (terms.size() > (size_t)kTsMaxTerms) return false;
    }
    bytes->clear();
    hdr->clear();
    for (auto &t : terms) {
        if (bytes->size() + t.size() > (size_t)kTsTermBytes) return false;
        hdr->push_back((uint32_t)bytes->size() | (uint32_t)t.size() << 16);
        bytes->insert(bytes->end(), t.begin(), t.end());
    }
    return true;
}

bool ts_has_nulls(const qeh_column &c) { return c.validity && c.null_count != 0; }

int ts_check_side(const TsSide &s, int64_t n, const char *what) {
    if (s.mode < QEH_TS_PLAIN || s.mode > QEH_TS_TSQUERY) return fail(QEH_E_INVALID, std::string("@@: bad mode of the ") + what);
    if (!s.col) {
        if (s.lit_len < 0 || s.lit_len > 0x7FFFFFFFll || (s.lit_len > 0 && !s.lit))
            return fail(QEH_E_INVALID, "Utf8 literal without bytes");
        return QEH_OK;
    }
    QEH_TRY(check_column(*s.col, "@@"));
    if (s.col->dtype != QEH_DT_UTF8)
        return fail(QEH_E_TYPE, std::string("@@ ") + what + " operand must be " +
                                    (what[0] == 'l' ? "tsvector (string)" : "tsquery (string)"));
    if (s.col->length != n) return fail(QEH_E_INVALID, "@@: operands have different lengths");
    if (n > 0 && !s.col->offsets) return fail(QEH_E_INVALID, "Utf8 column without offsets");
    return QEH_OK;
}

}  // namespace

int ts_match(qeh_ctx *ctx, const TsSide &doc, const TsSide &query, int64_t n, qeh_column *out) {
    std::memset(out, 0, sizeof(*out));
    if (n < 0) return fail(QEH_E_INVALID, "@@: negative length");
    QEH_TRY(ts_check_side(doc, n, "left"));
    QEH_TRY(ts_check_side(query, n, "right"));
    if (n > 0)  // a literal stands in every row
        for (const TsSide *s : {&doc, &query})
            if (!s->col && std::any_of(s->lit, s->lit + s->lit_len, [](uint8_t c) { return c >= 0x80; })) return ts_non_ascii();
    const bool nullable = (doc.col && ts_has_nulls(*doc.col)) || (query.col && ts_has_nulls(*query.col));
    QEH_TRY(alloc_column(ctx, QEH_DT_BOOL, n, nullable, out));
    out->null_count = nullable ? -1 : 0;
    if (n == 0) return QEH_OK;
    void *scr = nullptr;
    int s = scratch_zeroed(ctx, 64, &scr);
    DevBuf lits[2], table;
    std::vector<uint8_t> tb;  // host copies live until the flag is read
    std::vector<uint32_t> th;
    const bool stream = s == QEH_OK && doc.col && !query.col && !std::getenv("QEH_NO_TS_STREAM") &&
                        ts_term_table(query.lit, query.lit_len, query.mode, &tb, &th);
    if (s == QEH_OK && stream) {
        // [kTsMaxTerms headers][term bytes]
        const size_t hb = (size_t)kTsMaxTerms * 4;
        s = table.alloc(ctx, hb + std::max<size_t>(tb.size(), 1));
        if (s == QEH_OK && !th.empty() &&
            (hipMemcpyAsync(table.p, th.data(), th.size() * 4, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
             hipMemcpyAsync(table.as<uint8_t>() + hb, tb.data(), tb.size(), hipMemcpyHostToDevice, ctx->stream) != hipSuccess))
            s = fail(QEH_E_HIP, "@@: hipMemcpyAsync failed");
        if (s == QEH_OK) {
            const qeh_column &c = *doc.col;
            const int grid = grid_for(ctx, n, kBlock, 8);
            const int32_t *offs = c.offsets + c.offset;
            const uint8_t *data = (const uint8_t *)c.values;
            const uint8_t *dtb = table.as<uint8_t>() + hb;
            const uint32_t *dth = table.as<uint32_t>();
            const ColRef valid = make_colref(c);
            uint64_t *ob = (uint64_t *)out->values, *ov = (uint64_t *)out->validity;
            uint64_t first[2] = {0, 0};  // the terms' first bytes (the literal is ASCII)
            for (uint32_t h : th) first[(tb[h & 0xFFFFu] & 127u) >> 6] |= 1ull << (tb[h & 0xFFFFu] & 63u);
            KernelTimer kt(ctx, "ts_match_stream");
#define QEH_TS_LAUNCH(M)                                                                                              \
    hipLaunchKernelGGL(k_ts_match_stream<M>, dim3(grid), dim3(kBlock), 0, ctx->stream, offs, data, valid, n, dtb, dth, \
                       (int)th.size(), (int)tb.size(), first[0], first[1], ob, ov, (uint32_t *)scr)
            if (doc.mode == QEH_TS_TSVECTOR) QEH_TS_LAUNCH(QEH_TS_TSVECTOR);
            else if (doc.mode == QEH_TS_TSQUERY) QEH_TS_LAUNCH(QEH_TS_TSQUERY);
            else QEH_TS_LAUNCH(QEH_TS_PLAIN);
#undef QEH_TS_LAUNCH
        }
    } else if (s == QEH_OK) {
        TsOperand op[2];
        for (int k = 0; k < 2 && s == QEH_OK; ++k) {
            const TsSide &sd = k == 0 ? doc : query;
            TsOperand &o = op[k];
            o = TsOperand{};
            o.mode = sd.mode;
            if (sd.col) {
                o.valid = make_colref(*sd.col);
                o.offs = sd.col->offsets + sd.col->offset;
                o.data = (const uint8_t *)sd.col->values;
            } else {
                s = lits[k].alloc(ctx, (size_t)std::max<int64_t>(sd.lit_len, 1));
                if (s == QEH_OK && sd.lit_len > 0 &&
                    hipMemcpyAsync(lits[k].p, sd.lit, (size_t)sd.lit_len, hipMemcpyHostToDevice, ctx->stream) != hipSuccess)
                    s = fail(QEH_E_HIP, "@@: hipMemcpyAsync failed");
                o.data = lits[k].as<uint8_t>();
                o.lit_len = (int32_t)sd.lit_len;
                o.is_lit = 1;
            }
        }
        if (s == QEH_OK) {
            KernelTimer kt(ctx, "ts_match_rows");
            hipLaunchKernelGGL(k_ts_match_rows, dim3(grid_for(ctx, (n + 63) / 64, kBlock / 64, 8)), dim3(kBlock), 0, ctx->stream,
                               op[0], op[1], n, (uint64_t *)out->values, (uint64_t *)out->validity, (uint32_t *)scr);
        }
    }
    if (s == QEH_OK && hipGetLastError() != hipSuccess) s = fail(QEH_E_HIP, "@@: kernel launch failed");
    uint32_t flag = 0;
    // the read also orders the release of the literal / term buffers after their reader
    if (s == QEH_OK) s = read_small(ctx, &flag, scr, 4);
    else (void)hipStreamSynchronize(ctx->stream);
    if (s == QEH_OK && flag) s = ts_non_ascii();
    if (s != QEH_OK) qeh_column_release(ctx, out);
    return s;
}

}  // namespace qeh

extern "C" int qeh_ts_match(qeh_ctx *ctx, const qeh_column *doc, int doc_mode, const qeh_column *query_col,
                            const char *query_lit, int64_t query_lit_len, int query_mode, qeh_column *out) {
    using namespace qeh;
    if (!ctx || !doc || !out) return fail(QEH_E_INVALID, "qeh_ts_match: bad argument");
    DeviceGuard dg(ctx->device);
    TsSide d, q;
    d.col = doc;
    d.mode = doc_mode;
    q.col = query_col;
    q.lit = (const uint8_t *)query_lit;
    q.lit_len = query_col ? 0 : query_lit_len;
    q.mode = query_mode;
    return ts_match(ctx, d, q, doc->length, out);
}
