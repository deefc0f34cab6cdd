// The fused pipeline of qeh_join_filter_aggregate: its plan (k_fused_plan) and its one-workgroup
// finalize (k_fused_finish) around phases A and B of the slice pipeline (k_aggregate.hip).  Exports
// fused_join_filter_aggregate (aggregate.h).
#include <algorithm>
#include <cstdlib>

#include "aggregate.h"

namespace qeh {

// ---- fused pipeline: the plan -----------------------------------------------------------------
// The build rows (key, group key) take the probe rows' route: phase A's prologue groups them by slice
// (4-B items), and phase B builds each slice's entries in LDS from them instead of loading a join table
// from HBM.  No table is written, there are no scattered 2-B stores (the XCD-split insert read every
// key 8 times, 1.2 GB per query), and nothing of the build runs beside phase A.
// mm[0] = build key, mm[1] = group key ranges; nd = build rows (no NULLs allowed); dim_items = the
// build-row region buffer's size in items; st = the status words (zeroed here, [5] = the verdict).
// One launch ahead of phase A: workgroup 0 reduces the build key / group key partial min / max
// (part[c * nb + w], c = 0 key, 1 group key) and writes the plan and the zeroed status words; every
// workgroup initialises its share of the aggregate states.
__global__ __launch_bounds__(1024) void k_fused_plan(const MinMax *__restrict__ part, int nb, SlicePlanIn pi, int64_t g_cap,
                                                     int64_t nd, uint64_t dim_items, FusedPlan *out, uint32_t *__restrict__ st,
                                                     uint64_t *__restrict__ states, int64_t G, AggSpecs specs) {
    const int64_t words = (int64_t)specs.shards * specs.n_slots * G;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < words; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t slot = (i / G) % specs.n_slots;
        uint64_t v = 0;
        for (int a = 0; a < specs.n; ++a)
            if (specs.a[a].val_slot == slot) v = (uint64_t)agg_init_value(specs.a[a].kind);
        states[i] = v;
    }
    if (blockIdx.x != 0) return;
    __shared__ MinMax sm[2][16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int c = 0; c < 2; ++c) {
        int64_t mn = INT64_MAX, mx = INT64_MIN;
        uint64_t cnt = 0;
        uint32_t bad = 0;
        for (int i = threadIdx.x; i < nb; i += blockDim.x) {
            const MinMax q = part[(int64_t)c * nb + i];
            mn = q.mn < mn ? q.mn : mn;
            mx = q.mx > mx ? q.mx : mx;
            cnt += q.cnt;
            bad |= q.bad;
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const int64_t a = __shfl_xor(mn, d, 64), b2 = __shfl_xor(mx, d, 64);
            const uint64_t cc = __shfl_xor(cnt, d, 64);
            const uint32_t bb = __shfl_xor(bad, d, 64);
            mn = a < mn ? a : mn;
            mx = b2 > mx ? b2 : mx;
            cnt += cc;
            bad |= bb;
        }
        if (lane == 0) sm[c][wave] = MinMax{mn, mx, cnt, bad};
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    MinMax mm[2];
    for (int c = 0; c < 2; ++c) {
        mm[c] = sm[c][0];
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) {
            const MinMax q = sm[c][w];
            mm[c].mn = q.mn < mm[c].mn ? q.mn : mm[c].mn;
            mm[c].mx = q.mx > mm[c].mx ? q.mx : mm[c].mx;
            mm[c].cnt += q.cnt;
            mm[c].bad |= q.bad;
        }
    }
    FusedPlan p{};
    p.sp = plan_slices(pi, mm[0].mn, mm[0].mx, (int64_t)mm[0].cnt, mm[1].mn, mm[1].mx, (int64_t)mm[1].cnt);
    const bool full = (int64_t)mm[0].cnt == nd && (int64_t)mm[1].cnt == nd && !mm[0].bad && !mm[1].bad;
    p.gmin = mm[1].mn;
    p.ngroups = full ? (int64_t)((uint64_t)mm[1].mx - (uint64_t)mm[1].mn + 1ull) : 0;
    p.dcap = p.sp.F > 0 ? dim_items / ((uint64_t)pi.grid * p.sp.F) / 4 * 4 : 0;
    p.sp.ok = p.sp.ok && full && p.ngroups >= 1 && p.ngroups <= g_cap && p.ngroups < 0xFFFF && p.dcap >= 4;
    *out = p;
    for (int i = 0; i < 8; ++i) st[i] = 0u;
    st[5] = p.sp.ok ? 1u : 0u;
}

// After phase B (shard copies folded): one workgroup compacts the non-empty group slots, writes the
// output keys, aggregates and validity words (zeroed here first) and the group count (*total).
__global__ __launch_bounds__(1024) void k_fused_finish(const uint64_t *__restrict__ states, int64_t G, KeyCols keys,
                                                       const uint32_t *__restrict__ rep, AggSpecs specs, OutCols outs,
                                                       uint64_t *__restrict__ total) {
    __shared__ uint32_t pos[kSliceStateWords];
    __shared__ uint32_t vbits[kMaxGroupKeys + kMaxAggs][kSliceStateWords / 32];  // validity, built in LDS
    __shared__ uint32_t wsum[16];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int nout = keys.n + specs.n;
    const int64_t vwords = (G + 31) / 32;
    for (int c = 0; c < nout; ++c)
        for (int64_t w = t; w < vwords; w += blockDim.x) vbits[c][w] = 0u;
    const int64_t per = (G + 1023) / 1024, g0 = (int64_t)t * per, g1 = g0 + per < G ? g0 + per : G;
    uint32_t c = 0;
    for (int64_t g = g0; g < g1; ++g) c += states[g] != 0;
    const uint32_t incl = wave_incl_scan(c);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    uint32_t base = incl - c, all = 0;
    for (int w = 0; w < 16; ++w) {
        base += w < wave ? wsum[w] : 0u;
        all += wsum[w];
    }
    for (int64_t g = g0; g < g1; ++g) {
        pos[g] = base;
        base += states[g] != 0;
    }
    if (t == 0) *total = all;
    __syncthreads();  // validity bits zeroed, positions known
    // values by plain stores, validity bits in LDS (written out once below)
    auto put = [&](int c, int64_t p, int64_t payload, bool valid) {
        OutCol o = outs.c[c];
        if (o.validity && valid) atomicOr(&vbits[c][p >> 5], 1u << (p & 31));
        o.validity = nullptr;
        write_value(o, p, payload, true);
    };
    for (int64_t g = t; g < G; g += blockDim.x) {
        const uint64_t rows = states[g];
        if (!rows) continue;
        const int64_t p = pos[g];
        for (int k = 0; k < keys.n; ++k) {
            const int64_t r = rep[g];
            put(k, p, load_i64(keys.c[k], r), col_valid(keys.c[k], r));
        }
        for (int a = 0; a < specs.n; ++a) {
            const AggSpec sp = specs.a[a];
            const uint64_t cnt = sp.cnt_slot ? states[(int64_t)sp.cnt_slot * G + g] : rows;
            const int64_t v = sp.kind == AK_COUNT ? 0 : (int64_t)states[(int64_t)sp.val_slot * G + g];
            const int o = keys.n + a;
            const bool i32 = sp.in_type == QEH_DT_INT32;
            const bool flt = sp.in_type == QEH_DT_FLOAT32 || sp.in_type == QEH_DT_FLOAT64;
            switch (sp.func) {
                case QEH_AGG_COUNT: put(o, p, (int64_t)cnt, true); break;
                case QEH_AGG_SUM: put(o, p, i32 ? (int64_t)(int32_t)v : v, cnt != 0); break;
                case QEH_AGG_AVG: {
                    double sm = flt ? as_f64(v) : (double)(i32 ? (int64_t)(int32_t)v : v);
                    put(o, p, f64_bits(cnt ? sm / (double)cnt : 0.0), cnt != 0);
                    break;
                }
                default: put(o, p, flt ? f64_bits(f64_from_order_key(v)) : v, cnt != 0); break;
            }
        }
    }
    __syncthreads();
    for (int c = 0; c < nout; ++c)
        if (outs.c[c].validity)
            for (int64_t w = t; w < vwords; w += blockDim.x) outs.c[c].validity[w] = vbits[c][w];
}

// ---- the fused pipeline (one bounded integer group key, unique Int64 build keys) ----------------
// Everything on the main queue, one host round trip per query (the status words after the finalize):
//   build key / group key min-max -> k_fused_plan (slice shape, group slots, status words zeroed)
//   -> states zeroed -> phase A (prologue: output group keys and the build rows grouped by slice into
//   per-(workgroup, slice) regions, 4 B each; then the probe rows with EARLY loads and the ragged tail
//   as a partial last tile) -> phase B (each slice's entries built in LDS from its build rows,
//   duplicate keys flagged) -> fold / compact / finalize.
// Returns kFusedNotEligible when the shape does not qualify (checked on the host) or the device plan,
// a region overflow or a duplicate build key rejected the run (outputs released): the caller runs
// the general path.
int fused_join_filter_aggregate(qeh_ctx *ctx, const ColSet &cols, int64_t n, const PredPlan &pp,
                                const AggSpecs &specs_in, int key_col, const qeh_column &bk, const qeh_column &gk,
                                qeh_column *out_keys, qeh_column *out_aggs, int64_t *out_groups) {
    if (std::getenv("QEH_NO_FUSED") || std::getenv("QEH_NO_SLICES")) return kFusedNotEligible;
    const size_t timing_mark = ctx->timing_pending.size();
    const bool bk_nulls = bk.validity && bk.null_count != 0, gk_nulls = gk.validity && gk.null_count != 0;
    if (bk.dtype != QEH_DT_INT64 || bk_nulls || (gk.dtype != QEH_DT_INT64 && gk.dtype != QEH_DT_INT32) || gk_nulls)
        return kFusedNotEligible;
    const int64_t nd = bk.length;
    if (nd <= 0 || nd >= ((int64_t)1 << 32) || gk.length != nd) return kFusedNotEligible;
    FastIn in;
    int nterms, nacol;
    if (!fast_cols_eligible(cols, pp, key_col, specs_in, &in, &nterms, &nacol) || nacol > 2 ||
        (nacol == 2 && std::getenv("QEH_NO_FUSED_AGG2")))
        return kFusedNotEligible;
    // phase A: one 1024-thread workgroup per CU (two aggregate columns: 18-B items, half tiles)
    const int64_t tile_rows = nacol == 2 ? (int64_t)SliceShape<2, true>::TILE
                                         : (nacol ? SliceShape<1, true>::TILE : SliceShape<0, true>::TILE);
    const int chunk = nacol == 2 ? SliceShape<2, true>::CH : (nacol ? SliceShape<1, true>::CH : SliceShape<0, true>::CH);
    const int64_t n_tiles = n / tile_rows, tail = n - n_tiles * tile_rows;
    if (n_tiles == 0) return kFusedNotEligible;
    AggSpecs specs = specs_in;
    const int64_t g_cap = std::min<int64_t>(kSliceStateWords / std::max(specs.n_slots, 1), 0xFFFE);
    const int64_t Gs = g_cap;  // states and outputs for every possible slot; empty slots are dropped
    // one copy of the states: phase B folds each slice's LDS states into them once per workgroup, so
    // same-address contention is low and the shard fold launch is not worth its place in the chain
    // (A/B on one box, profiles/r04/ab_early_shape.txt); QEH_FUSED_SHARDS=1 restores the copies
    specs.shards = 1;
    if (std::getenv("QEH_FUSED_SHARDS"))
        while (specs.shards < 64 && (size_t)specs.n_slots * Gs * 8 * specs.shards * 2 <= (8u << 20)) specs.shards *= 2;
    const int64_t n_all = n_tiles + (tail ? 1 : 0);
    const int grid = (int)std::min<int64_t>({(int64_t)ctx->props.multiProcessorCount, n_all,
                                             (int64_t)kMaxSliceGrid});
    const uint64_t tiles_per_wg = (uint64_t)((n_all + grid - 1) / grid);

    DevBuf mm, plan, ditems, dcount, kbuf, vbuf, vbuf2, cbuf, states, errw, gkeys, rep;
    SlicePlanIn pi{};
    pi.min_bytes = slice_min_bytes();
    pi.grid = grid;
    pi.n_slots = specs.n_slots;
    pi.sparse_ok = direct_sparse_allowed() ? 1 : 0;
    pi.chunk = chunk;
    pi.alloc_items = tiles_per_wg * grid * (uint64_t)tile_rows * 5 / 4 + (uint64_t)grid * kSliceMaxF * (256 + 2 * chunk);
    // build rows: uniform keys over the slices, +25 %, and per-region slack
    const uint64_t dim_items = (uint64_t)nd * 5 / 4 + (uint64_t)grid * kSliceMaxF * 64;
    if (dim_items >= (1ull << 32)) return kFusedNotEligible;  // phase B's region bases are 32-bit
    const uint64_t nreg_max = (uint64_t)grid * kSliceMaxF;
    QEH_TRY(mm.alloc(ctx, sizeof(MinMax) * 2 * (size_t)minmax_partials_max_blocks(ctx) + 16));  // the partials
    QEH_TRY(plan.alloc(ctx, sizeof(FusedPlan)));
    QEH_TRY(ditems.alloc(ctx, dim_items * 4 + 64));
    QEH_TRY(dcount.alloc(ctx, nreg_max * 4 + 64));
    QEH_TRY(kbuf.alloc(ctx, pi.alloc_items * 2 + 64));
    if (nacol) QEH_TRY(vbuf.alloc(ctx, pi.alloc_items * 8 + 64));
    if (nacol > 1) QEH_TRY(vbuf2.alloc(ctx, pi.alloc_items * 8 + 64));
    QEH_TRY(cbuf.alloc(ctx, nreg_max * 4 + 64));
    QEH_TRY(states.alloc(ctx, (size_t)specs.shards * specs.n_slots * Gs * 8));
    // status words (zeroed by k_fused_plan): [0] kernel error bits, [1] region overflow, [2..3] groups,
    // [4] duplicate build key, [5] the device plan's verdict
    QEH_TRY(errw.alloc(ctx, 32));
    QEH_TRY(gkeys.alloc(ctx, (size_t)Gs * 8));
    QEH_TRY(rep.alloc(ctx, (size_t)Gs * 4));
    uint32_t *st = errw.as<uint32_t>();
    SliceRegions rg{};
    rg.key = kbuf.as<uint16_t>();
    rg.val = nacol ? vbuf.as<int64_t>() : nullptr;
    rg.val2 = nacol > 1 ? vbuf2.as<int64_t>() : nullptr;
    rg.count = cbuf.as<uint32_t>();
    rg.overflow = st + 1;
    FusedPlan *dplan = plan.as<FusedPlan>();
    {
        KernelTimer kt(ctx, "fused_build");
        const qeh_column both[2] = {bk, gk};
        int nb = 0;
        QEH_TRY(columns_minmax_partials(ctx, both, 2, mm.as<MinMax>(), &nb));
        const int gp = (int)std::max<int64_t>(1, std::min<int64_t>(ctx->props.multiProcessorCount,
                                                                   (specs.shards * specs.n_slots * Gs + 4095) / 4096));
        hipLaunchKernelGGL(k_fused_plan, dim3(gp), dim3(1024), 0, ctx->stream, mm.as<MinMax>(), nb, pi, g_cap, nd, dim_items,
                           dplan, st, states.as<uint64_t>(), Gs, specs);
    }
    QEH_HIP(hipGetLastError());
    FusedPro fp{};
    fp.dk = (const int64_t *)bk.values + bk.offset;
    fp.dg = make_colref(gk);
    fp.nd = nd;
    fp.ditems = ditems.as<uint32_t>();
    fp.dcount = dcount.as<uint32_t>();
    fp.status = st;
    fp.gkeys = gkeys.p;
    fp.rep = rep.as<uint32_t>();
    fp.G = Gs;
    fp.as32 = gk.dtype == QEH_DT_INT32 ? 1 : 0;
    fp.plan = dplan;
    launch_slice_partition_early(ctx, in, pp, nterms, nacol, n_tiles, tail, grid, rg, &dplan->sp, fp);
    {
        KernelTimer ktb(ctx, "slice_probe");
        DimSlices dim{ditems.as<uint32_t>(), dcount.as<uint32_t>(), st + 4, dplan};
        // items loaded two per lane (PV, default; QEH_FUSED_PV=0: one per lane)
        static const bool pv = !(std::getenv("QEH_FUSED_PV") && std::atoi(std::getenv("QEH_FUSED_PV")) == 0);
        launch_slice_probe_dim(ctx, rg, grid, in, specs, Gs, states.as<uint64_t>(), dim, nacol, pv);
    }
    QEH_HIP(hipGetLastError());
    // fold the shard copies (when there are several), then one workgroup compacts, writes the outputs
    // and the group count (st[2..3])
    if (specs.shards > 1) states_fold(ctx, states.as<uint64_t>(), Gs, specs);
    QEH_HIP(hipGetLastError());
    qeh_column kc{};
    kc.dtype = gk.dtype;
    kc.length = Gs;
    kc.values = gkeys.p;
    KeyCols keys{};
    keys.n = 1;
    keys.c[0] = make_colref(kc);
    OutCols oc{};
    int made = 0;
    auto cleanup = [&]() {
        for (int i = 0; i < made; ++i) qeh_column_release(ctx, i == 0 ? &out_keys[0] : &out_aggs[i - 1]);
        made = 0;
    };
    for (int i = 0; i < 1 + specs.n; ++i) {
        qeh_column *c = i == 0 ? &out_keys[0] : &out_aggs[i - 1];
        int dt;
        bool nullable;
        if (i == 0) {
            dt = gk.dtype;
            nullable = false;
        } else {
            const AggSpec &sp = specs.a[i - 1];
            dt = agg_output_type(sp.func, sp.in_type);
            nullable = sp.func != QEH_AGG_COUNT;
        }
        const int s = alloc_column(ctx, dt, Gs, nullable, c);
        if (s != QEH_OK) {
            cleanup();
            return s;
        }
        ++made;
        oc.c[i].values = c->values;
        oc.c[i].validity = (uint32_t *)c->validity;
        oc.c[i].dtype = dt;
    }
    {
        KernelTimer kt(ctx, "aggregate_finalize");
        hipLaunchKernelGGL(k_fused_finish, dim3(1), dim3(1024), 0, ctx->stream, states.as<uint64_t>(), Gs, keys,
                           rep.as<uint32_t>(), specs, oc, (uint64_t *)(st + 2));
    }
    uint32_t sw[8];
    int s = hipGetLastError() == hipSuccess ? QEH_OK : fail(QEH_E_HIP, "fused join-aggregate: launch failed");
    if (s == QEH_OK) s = read_small(ctx, sw, errw.p, 32);  // the one host round trip of the query
    if (s == QEH_OK && !sw[0] && (!sw[5] || sw[1] || sw[4])) s = kFusedNotEligible;  // plan, overflow, duplicates
    if (s == kFusedNotEligible && !sw[5]) {
        // the device plan declined: every kernel of this call returned at once, so its timing records
        // are not a query's phases (the general path that follows records its own)
        for (size_t i = timing_mark; i < ctx->timing_pending.size(); ++i) ctx->timing_pending[i].name += "_declined";
    }
    if (s == QEH_OK) s = kernel_error_status(sw[0], "aggregate");
    if (s != QEH_OK) {
        cleanup();
        return s;
    }
    const int64_t out_n = (int64_t)((uint64_t)sw[2] | ((uint64_t)sw[3] << 32));
    for (int i = 0; i < 1 + specs.n; ++i) {
        qeh_column *c = i == 0 ? &out_keys[0] : &out_aggs[i - 1];
        c->length = out_n;
        c->null_count = c->validity ? -1 : 0;
    }
    *out_groups = out_n;
    return QEH_OK;
}

}  // namespace qeh
