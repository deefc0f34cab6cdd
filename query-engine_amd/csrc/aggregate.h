// Host interface between the aggregate units: k_aggregate.hip (the general aggregate, the LDS-slice
// pipeline, the distributed forms and the top-level fused entry), k_agg_probe.hip (the fast and
// bucket-range probes), k_slice_join.hip (the slice pipeline's materialising join) and k_agg_fused.hip
// (the fused pipeline).  Every kernel is instantiated in one unit only; the others reach it through
// the launchers declared here.
#pragma once
#include <cstdlib>
#include <type_traits>

#include "agg_device.h"

namespace qeh {

struct PredPlan {
    int mode = PM_NONE;
    PredTerms terms{};
    DevProgram prog{};
};

inline bool fast_col_ok(const ColRef &c) {
    return (c.dtype == QEH_DT_INT64 || c.dtype == QEH_DT_FLOAT64) && c.validity == nullptr &&
           ((uintptr_t)c.values & 15) == 0;
}

inline uint64_t table_bytes(const HashTable &t) {
    if (t.kind == TK_DIRECT) return t.range * (t.payload16 ? 2 : 4);
    if (t.kind == TK_PACKED) return (t.mask + 1) * 8;
    if (t.kind == TK_BUCKET) return t.nbkt * 64;
    return (t.mask + 1) * 16;
}

// Smallest join table (bytes) worth the two-phase slice pipeline (QEH_SLICE_MIN_BYTES, read per call):
// below ~1.5 L2s the single pass's lookups mostly hit L2 and it wins.
inline uint64_t slice_min_bytes() {
    const char *e = std::getenv("QEH_SLICE_MIN_BYTES");
    return e ? std::strtoull(e, nullptr, 10) : 6ull << 20;
}

// The fast kernels' (NTERMS, NACOL, NT) template parameters from their runtime values: calls
// f(integral_constant<int, nterms>, integral_constant<int, nacol>, bool_constant<nt>) for nterms in
// 0..2 and nacol in 0..MAXNA (anything above counts as MAXNA).
template <int MAXNA = 2, class F>
inline void dispatch_fast(int nterms, int nacol, bool nt, F &&f) {
    auto by_nacol = [&](auto NTV, auto NTB) {
        if (nacol == 0) f(NTV, std::integral_constant<int, 0>{}, NTB);
        else if (MAXNA == 1 || nacol == 1) f(NTV, std::integral_constant<int, 1>{}, NTB);
        else f(NTV, std::integral_constant<int, MAXNA>{}, NTB);
    };
    auto by_nterms = [&](auto NTB) {
        if (nterms == 0) by_nacol(std::integral_constant<int, 0>{}, NTB);
        else if (nterms == 1) by_nacol(std::integral_constant<int, 1>{}, NTB);
        else by_nacol(std::integral_constant<int, 2>{}, NTB);
    };
    if (nt) by_nterms(std::true_type{});
    else by_nterms(std::false_type{});
}

// ---- k_aggregate.hip ---------------------------------------------------------------------------
int agg_output_type(int func, int in_type);
// rows [done, n) (the ragged tail past a fast path's full tiles) through the generic kernel
void launch_tail(qeh_ctx *ctx, const ColSet &cols, int64_t n, int64_t done, const PredPlan &pp, const GidSource &src,
                 const AggSpecs &specs, int64_t G, uint64_t *states, uint32_t *err, size_t lds_bytes);
// the shard copies of small state tables folded into copy 0 (k_states_fold), on the main queue
void states_fold(qeh_ctx *ctx, uint64_t *states, int64_t Gs, const AggSpecs &specs);
void fill_i64(qeh_ctx *ctx, int grid, int block, int64_t *p, int64_t n, int64_t v);
// Phase A (k_slice_partition) over n_tiles full tiles.  gid_table != nullptr: MODE 1 (group-range slices,
// `range` = groups).  timer: the launch's timing record, nullptr when the caller times it under a name
// of its own.
void launch_slice_partition(qeh_ctx *ctx, const FastIn &in, const PredPlan &pp, int nterms, int nacol, int64_t kmin,
                            uint64_t range, int64_t n_tiles, int grid, const SliceRegions &rg_in, hipStream_t stream,
                            const HashTable *gid_table = nullptr, const SlicePlan *dplan = nullptr,
                            const char *timer = "slice_partition");
// Phase A of the fused pipeline and the items forms (EARLY loads, the prologue, the ragged tail as a
// partial last tile), timed as "slice_partition" on the main queue.
void launch_slice_partition_early(qeh_ctx *ctx, const FastIn &in, const PredPlan &pp, int nterms, int nacol,
                                  int64_t n_tiles, int64_t tail_rows, int grid, const SliceRegions &rg,
                                  const SlicePlan *dplan, const FusedPro &fp);
// Phase B with each slice's entries built in LDS from build-row items (k_slice_probe's DIM form), on the
// main queue under the caller's timer.  pairs: items loaded two per lane (one aggregate column only).
// Used by the fused pipeline; the items forms (k_aggregate.hip) still launch the same instantiations
// themselves.
void launch_slice_probe_dim(qeh_ctx *ctx, const SliceRegions &rg, int nreg, const FastIn &in, const AggSpecs &specs,
                            int64_t G, uint64_t *states, const DimSlices &dim, int nacol, bool pairs);

// ---- k_agg_probe.hip ---------------------------------------------------------------------------
// QEH_NT_LOADS (non-temporal fact-column loads, default on), read once per process
int fast_nt_mode();
// Eligibility of the specialised probe kernels; fills the kernel's view.
// `key_col`: the column read as FastIn::key (join probe key or group key).
bool fast_cols_eligible(const ColSet &cols, const PredPlan &pp, int key_col, const AggSpecs &specs, FastIn *inp,
                        int *nterms_out, int *nacol_out);
bool fast_eligible(const ColSet &cols, const PredPlan &pp, const GidSource &src, const AggSpecs &specs, FastIn *inp,
                   int *nterms_out, int *nacol_out);
// The fused probe's fast path: returns true when it launched (full tiles by
// k_join_agg_fast or the bucket-range probe, the ragged tail by the generic kernel).
bool try_fast_join(qeh_ctx *ctx, const ColSet &cols, int64_t n, const PredPlan &pp, const GidSource &src,
                   const AggSpecs &specs, int64_t G, uint64_t *states, uint32_t *err, size_t lds_bytes, int per_cu);

// ---- k_slice_join.hip --------------------------------------------------------------------------
// LDS-slice materialising INNER join of one probe payload and one Int64 build
// payload; kSliceJoinNotEligible when the shapes do not fit.
constexpr int kSliceJoinNotEligible = -1;
int slice_join_materialise(qeh_ctx *ctx, const qeh_column &probe_key, const qeh_column &probe_val,
                           const qeh_column &build_key, const qeh_column &build_val, qeh_column *out_probe,
                           qeh_column *out_build, int64_t *out_rows);

// ---- k_agg_fused.hip ---------------------------------------------------------------------------
// The fused pipeline (one bounded integer group key, unique Int64 build keys); kFusedNotEligible when
// the shape does not qualify or the device rejected the run (outputs released): the caller runs the
// general path.
constexpr int kFusedNotEligible = -4;
int fused_join_filter_aggregate(qeh_ctx *ctx, const ColSet &cols, int64_t n, const PredPlan &pp,
                                const AggSpecs &specs_in, int key_col, const qeh_column &bk, const qeh_column &gk,
                                qeh_column *out_keys, qeh_column *out_aggs, int64_t *out_groups);

}  // namespace qeh
