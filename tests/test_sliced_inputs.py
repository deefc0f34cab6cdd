"""Every operator on sliced columns (non-zero Arrow offset, unknown NULL count).

Each case builds its columns with sliced.make(): the logical rows sit inside a parent whose other rows
are poison (type MIN / MAX and repeated keys, NaN / inf, complemented Bools and validity bits, long
distinct strings).  The device gets `ctx.slice(parent, lead, n)` views with leads 1, 2, 8 and 67 (the
columns of one call get different ones, sliced.CYCLES); the reference is the CPU oracle, or a numpy
restatement where the oracle has no such entry point, on the logical rows.  Comparisons are exact:
float inputs are whole numbers, so sums do not depend on their order.

test_inputs_discriminate (no GPU) shows for every case that the reference's answer changes under each
of three wrong readings of the parent: (a) a column's values taken from parent rows [0, n), (b) a
column's validity read from bit 0, (c) a table read one row past its end.  (a) and (b) are applied to
one column at a time, (c) to one table at a time.  A kernel that makes one of these mistakes on any
column therefore fails its case.  The few (case, column) pairs where a reading cannot change the
answer carry their reason in Case.exempt.

Row counts: 20 011 for the generic kernels (several blocks and a ragged tail), two slice tiles plus 17
rows for the join-aggregate sites (as test_agg_dispatch.py), 123 457 for the outer slice probe and
2^20 + 17 for the payload sort's MSD passes (reference: numpy's stable lexsort)."""
import zlib

import numpy as np
import pytest

import oracle_bind as ob
import sliced as S
from sliced import make, multiset, ordered, plain
from qe_hip import AggregateFunction as AF
from qe_hip import BinaryOp, UnaryExpr, UnaryOp, abi, binop, col, lit
from qe_hip.plan import WindowFunctionType as WF
from test_agg_dispatch import SITES, SLICE_TILE

N = 20_011
N_JOINAGG = 2 * SLICE_TILE + 17
N_OUTER_SLICE = 123_457
N_MSD_SORT = 2 ** 20 + 17
I64, I32, F64, F32 = np.int64, np.int32, np.float64, np.float32


class Case:
    """cols: the sliced columns; fn(B, h) runs the operator on backend B over the handles h (one per
    column, same order) and returns a list of canonical results.  env: switches that force a path;
    ran / absent: timing records that must (not) show up when every column is 16-B aligned.
    exempt: {(reading, column or table): reason} for readings that cannot change the answer."""

    def __init__(self, cols, fn, env=None, ran=(), absent=(), exempt=None):
        self.cols, self.fn, self.env, self.ran, self.absent = cols, fn, env or {}, tuple(ran), tuple(absent)
        self.exempt = exempt or {}


CASES = {}


def case(name):
    def reg(build):
        assert name not in CASES
        CASES[name] = build
        return build
    return reg


def rng(name, lead):
    return np.random.default_rng(zlib.crc32(name.encode()) + lead)


def ints(r, lo, hi, n, dt=I64):
    return r.integers(lo, hi, n).astype(dt)


def whole(r, n, dt=F64):
    return r.integers(-50, 50, n).astype(dt)


def mask(r, n, p=0.1, last=True):
    """validity with a fixed first and last bit: the poison bits next to the slice are their complements"""
    m = r.random(n) > p
    m[0], m[-1] = True, last
    return m


def key_values(r, kind, n):
    if kind == "int64":
        return ints(r, -500, 500, n)
    if kind == "int32":
        return ints(r, -500, 500, n, I32)
    if kind == "float64":
        return np.round(r.standard_normal(n), 1)
    if kind == "float32":
        return np.round(r.standard_normal(n), 1).astype(F32)
    return r.random(n) > 0.3


# ---- hash_aggregate / filter_aggregate ------------------------------------------------------------
# columns: 0 key, 1 v Float64 (whole numbers), 2 w Int64, 3 b Bool, 4 i Int32, 5 x Int64 (predicate)
AGGS = [(AF.Sum, 1), (AF.Count, 1), (AF.Avg, 1), (AF.Min, 1), (AF.Max, 1), (AF.Sum, 2), (AF.Min, 2), (AF.Max, 2),
        (AF.Count, 3), (AF.Sum, 4), (AF.Min, 4), (AF.Max, 4), (AF.Count, 0), (AF.Count, 5)]
COUNT_ONLY = "COUNT reads a column's validity, never its values"


def agg_columns(name, lead, kind, nullable, bool_in_predicate=False):
    L, r = S.lead_cycle(lead), rng(name, lead)
    m = (lambda: mask(r, N)) if nullable else (lambda: None)
    b, x = r.random(N) > 0.5, ints(r, 0, 100, N)
    # the first row and the row after the slice pass the predicates (x > 49 AND b), so a NULL put on the
    # one or the other's inclusion shows
    b[0], b[-S.TRAIL], x[0] = True, False, 99
    bm = mask(r, N, last=not bool_in_predicate) if nullable else None
    return [make(key_values(r, kind, N), m(), L(), key=True), make(whole(r, N), m(), L()),
            make(ints(r, -10 ** 6, 10 ** 6, N), "buffer" if nullable else None, L()), make(b, bm, L()),
            make(ints(r, -1000, 1000, N, I32), m(), L()), make(x, None, L(), poison=[99, -(2 ** 63), 2 ** 63 - 1])]


def add_hash_aggregate(name, kind, nullable, env=None, key_idx=(0,)):
    @case(name)
    def build(lead):
        cols = agg_columns(name, lead, kind, nullable)

        def fn(B, h):
            gk, ga = B.hash_aggregate([h[i] for i in key_idx], h, AGGS)
            return [multiset(gk + ga)]
        ex = {("a", 3): COUNT_ONLY, ("a", 5): COUNT_ONLY}
        if not key_idx:
            ex[("a", 0)] = COUNT_ONLY
        return Case(cols, fn, env=env, exempt=ex)


for _kind in ("int64", "int32", "float64", "float32", "bool"):
    for _nullable in (False, True):
        add_hash_aggregate("hash_aggregate-%s-%s" % (_kind, "null" if _nullable else "nn"), _kind, _nullable)
for _nullable in (False, True):
    add_hash_aggregate("hash_aggregate-no_lds-int64-%s" % ("null" if _nullable else "nn"), "int64", _nullable,
                       env={"QEH_NO_LDS_GROUPBY": "1"})
    add_hash_aggregate("hash_aggregate-two_keys-%s" % ("null" if _nullable else "nn"), "int32", _nullable, key_idx=(0, 4))
    add_hash_aggregate("hash_aggregate-no_keys-%s" % ("null" if _nullable else "nn"), "int64", _nullable, key_idx=())

GT49 = binop(col(5), BinaryOp.Greater, lit(49))
PRED_GENERIC = GT49 & col(3)  # the Bool column's values decide rows
PRED_2 = binop(col(5), BinaryOp.Greater, lit(20)) & binop(col(2), BinaryOp.Less, lit(500_000))


def add_filter_aggregate(name, kind, nullable, pred, aggs, env=None, key_idx=(0,), exempt=None):
    @case(name)
    def build(lead):
        cols = agg_columns(name, lead, kind, nullable, bool_in_predicate=pred is PRED_GENERIC)

        def fn(B, h):
            gk, ga = B.filter_aggregate(h, pred, list(key_idx), aggs)
            return [multiset(gk + ga)]
        return Case(cols, fn, env=env, exempt=exempt)


for _kind in ("int64", "int32", "float64", "float32", "bool"):
    for _nullable in (False, True):
        add_filter_aggregate("filter_aggregate-%s-%s" % (_kind, "null" if _nullable else "nn"), _kind, _nullable,
                             PRED_GENERIC, AGGS)
add_filter_aggregate("filter_aggregate-no_lds-int64-null", "int64", True, PRED_GENERIC, AGGS, env={"QEH_NO_LDS_GROUPBY": "1"})
add_filter_aggregate("filter_aggregate-two_keys-null", "int64", True, PRED_GENERIC, AGGS, key_idx=(0, 4))
add_filter_aggregate("filter_aggregate-no_keys-null", "int64", True, GT49, AGGS, key_idx=(),
                     exempt={("a", 0): COUNT_ONLY, ("a", 3): COUNT_ONLY})
# the fast kernels: non-null 8-byte columns only, a predicate of 0, 1 or 2 column-literal terms
FAST_AGGS = [(AF.Sum, 1), (AF.Sum, 2), (AF.Count, 1), (AF.Min, 2), (AF.Max, 1)]
UNUSED = "the fast shape names 8-byte columns only; this column is not read"
for _t, _pred in ((0, None), (1, GT49), (2, PRED_2)):
    add_filter_aggregate("filter_aggregate-fast-%dterm" % _t, "int64", False, _pred, FAST_AGGS,
                         exempt={("a", j): UNUSED for j in ((3, 4, 5) if _t == 0 else (3, 4))})


# ---- join_filter_aggregate: the four sites of test_agg_dispatch.py ---------------------------------
N_DIM, KEY0 = 300, -40
JA_PRED = binop(col(0), BinaryOp.Greater, lit(49))
JA_AGGS = {1: [(AF.Sum, 3), (AF.Count, 3), (AF.Max, 3)], 2: [(AF.Sum, 3), (AF.Sum, 4), (AF.Count, 3), (AF.Min, 4)]}


def add_join_aggregate(name, site, nacol, null_key):
    @case(name)
    def build(lead):
        L, r = S.lead_cycle(lead), rng(name, lead)
        n = N_JOINAGG
        # probe: 0 x, 1 y, 2 join key, 3 v Int64, 4 w Float64 (whole); build: 5 key, 6 group key
        probe = [make(ints(r, 0, 100, n), None, L(), poison=[99, -(2 ** 63), 2 ** 63 - 1]), make(ints(r, 0, 100, n), None, L()),
                 make(ints(r, KEY0 - 10, KEY0 + N_DIM + 10, n), mask(r, n, 0.05, last=False) if null_key else None, L(),
                      poison=[KEY0 + 5, KEY0 - 100, KEY0 + N_DIM + 100]),
                 make(ints(r, -50, 50, n), None, L()), make(whole(r, n), None, L())]
        dk = r.permutation(N_DIM).astype(I64) + KEY0
        # rows next to the build slice: keys the probe has and the build lacks, so they add matches
        build_cols = [make(dk, None, L(), table=1, poison=[KEY0 - 3, KEY0 + N_DIM + 2, KEY0 - 7]),
                      make(ints(r, 0, 16, N_DIM) - 5, None, L(), key=True, table=1)]
        env, ran = SITES[site]
        if null_key:
            ran = ()

        def fn(B, h):
            gk, ga = B.join_filter_aggregate(h[:5], 2, JA_PRED, h[5], [h[6]], JA_AGGS[nacol])
            return [multiset(gk + ga)]
        names = ("fused_build", "slice_partition", "slice_probe", "bucket_parts")
        ex = {("a", 1): "y is not named by the one-term predicate"}
        if nacol == 1:
            ex[("a", 4)] = "w is not aggregated in this shape"
        return Case(probe + build_cols, fn, env=env, ran=ran, absent=[x for x in names if x not in ran], exempt=ex)


for _site in SITES:
    add_join_aggregate("join_filter_aggregate-%s" % _site, _site, 1 if _site == "bucket" else 2, False)
add_join_aggregate("join_filter_aggregate-null_probe_key", "fast", 2, True)


# ---- hash_join_inner / hash_join_outer ----------------------------------------------------------------
JT = {"inner": 0, "left": 1, "right": 2, "full": 3}


def add_join(name, jt, shape, env=None, ran=(), nb=1, n_probe=N, kdt=I64):
    """shape: unique (DIRECT build, unique keys; nullable probe key and payloads), embed (unique build,
    non-null 8-byte payloads: nb build columns), rec16 / rec32 (one narrow Int64 build column: 2-B / 4-B
    records), dups (repeated build keys, NULL keys on both sides, Int32 build key)."""
    @case(name)
    def build(lead):
        L, r = S.lead_cycle(lead), rng(name, lead)
        npr = n_probe
        if shape == "dups":
            nbuild = 2000
            bk = make(ints(r, 0, 300, nbuild, I32), mask(r, nbuild, last=False), L(), key=True, table=1)
            pk = make(ints(r, 0, 400, npr), mask(r, npr, 0.05, last=False), L(), poison=[7, -150, 550])
            bcols = [bk, make(ints(r, -9, 9, nbuild), None, L(), table=1), make(whole(r, nbuild), mask(r, nbuild), L(), table=1)]
            pcols = [pk, make(whole(r, npr), mask(r, npr, 0.2), L()), make(r.random(npr) > 0.5, None, L())]
        else:
            nbuild, span = (5000, 9000) if npr == N else (60_000, 300_000)
            bkv = (r.permutation(span)[:nbuild] + 1000).astype(kdt)
            pkv, pkm = ints(r, 0, span + 3000, npr, kdt), mask(r, npr, 0.05, last=False)
            # rows next to the build slice: keys the probe has and the build lacks
            missing = np.setdiff1d(pkv[pkm & (pkv >= 1000) & (pkv < 1000 + span)], bkv)[:3]
            bk = make(bkv, None, L(), table=1, poison=missing)
            pk = make(pkv, pkm, L(), poison=[bkv[5], -span // 2, span + span // 2])  # the row after the slice matches
            if shape == "unique":
                bcols = [make(ints(r, -5, 5, nbuild), mask(r, nbuild), L(), table=1), bk]
                pcols = [pk, make(whole(r, npr), mask(r, npr, 0.2), L())]
            elif shape == "embed":
                bcols = [bk, make(whole(r, nbuild), None, L(), table=1), make(ints(r, -9, 9, nbuild), None, L(), table=1)][:nb]
                pcols = [pk, make(r.random(npr) > 0.5, mask(r, npr), L())] if jt != "full" else \
                    [make(whole(r, npr), None, L()), make(ints(r, -5, 5, npr), None, L())]
            else:
                lo, hi = (-700, 700) if shape == "rec16" else (-(1 << 20), 1 << 20)
                bcols = [make(ints(r, lo, hi, nbuild), None, L(), table=1)]
                pcols = [make(whole(r, npr), None, L())]
        cols = [pk] + [c for c in pcols if c is not pk] + [bk] + [c for c in bcols if c is not bk]
        at = {id(c): i for i, c in enumerate(cols)}

        def fn(B, h):
            hp, hb = [h[at[id(c)]] for c in pcols], [h[at[id(c)]] for c in bcols]
            hpk, hbk = h[at[id(pk)]], h[at[id(bk)]]
            if jt == "inner":
                out = B.join_inner(hpk, hp, hbk, hb)
            elif jt == "right":  # the probe side is the preserved (right) one
                out = B.join_outer(JT[jt], hbk, hb, hpk, hp)
            else:
                out = B.join_outer(JT[jt], hpk, hp, hbk, hb)
            if jt == "left" and shape != "dups" and "QEH_OUTER_COMPACT" not in (env or {}):  # one row per probe row, in probe order
                return [ordered(out)]
            return [multiset(out)]
        return Case(cols, fn, env=env, ran=ran)


for _jt in ("inner", "left", "right", "full"):
    add_join("join-%s-unique" % _jt, _jt, "unique")
    add_join("join-%s-dups_nulls_int32" % _jt, _jt, "dups")
    for _nb in (1, 2, 3):
        add_join("join-%s-embed%d" % (_jt, _nb), _jt, "embed", nb=_nb)
    for _rec in ("rec16", "rec32"):
        add_join("join-%s-%s" % (_jt, _rec), _jt, _rec)
        if _jt != "inner":
            add_join("join-%s-outer_slice-%s" % (_jt, _rec), _jt, _rec, env={"QEH_OUTER_SLICE": "1"}, ran=("outer_slice",),
                     n_probe=N_OUTER_SLICE)
    if _jt != "inner":
        add_join("join-%s-outer_slice-int32_keys" % _jt, _jt, "rec16", env={"QEH_OUTER_SLICE": "1"}, ran=("outer_slice",),
                 n_probe=N_OUTER_SLICE, kdt=I32)
        add_join("join-%s-unique-compact" % _jt, _jt, "unique", env={"QEH_OUTER_COMPACT": "1"})


def add_prebuild_fallback(name, jt):
    """One narrow Int64 build column (the prebuilt 2-B records' shape) whose build key repeats and has
    NULLs: the records are abandoned for the general join table."""
    @case(name)
    def build(lead):
        L, r = S.lead_cycle(lead), rng(name, lead)
        nbuild = 5000
        bkv = (r.permutation(9000)[:nbuild] + 1000).astype(I64)
        bkv[::50] = bkv[1::50][:len(bkv[::50])]  # repeated keys
        pkv, pkm = ints(r, 0, 12_000, N), mask(r, N, 0.05, last=False)
        # the rows next to either slice carry keys of the other side, so reading them adds matches
        bk = make(bkv, mask(r, nbuild, 0.03, last=False), L(), table=1, poison=[pkv[0], -5000, 17_000])
        ba = make(ints(r, -700, 700, nbuild), None, L(), table=1)
        pk = make(pkv, pkm, L(), poison=[bkv[5], -6000, 18_000])
        pv = make(whole(r, N), None, L())

        def fn(B, h):
            out = B.join_outer(JT[jt], h[2], [h[3]], h[0], [h[1]]) if jt == "right" else \
                B.join_outer(JT[jt], h[0], [h[1]], h[2], [h[3]])
            return [multiset(out)]
        return Case([pk, pv, bk, ba], fn)


for _jt in ("left", "right", "full"):
    add_prebuild_fallback("join-%s-narrow_records_dup_null_build_keys" % _jt, _jt)


# ---- sort ------------------------------------------------------------------------------------------------
def sort_key(r, kind, n, nullable, L, p=0.1, span=1000):
    m = mask(r, n, p) if nullable else None
    if kind == "int64":
        return make(ints(r, -span, span, n), m, L())
    if kind == "int32":
        return make(ints(r, -span, span, n, I32), m, L())
    if kind == "float64":  # -inf first: the row after the slice sorts to the front
        return make(np.round(r.standard_normal(n), 1), m, L(), poison=[-np.inf, np.nan, np.inf, -0.0])
    return make(np.array(["k%02d" % x * (1 + x % 3) for x in r.integers(0, 40, n)], dtype=object), m, L())


def add_sort(name, kinds, nullable, how="plain", env=None, asc=None, n=N, ran=(), span=1000):
    @case(name)
    def build(lead):
        L, r = S.lead_cycle(lead), rng(name, lead)
        cols = [sort_key(r, k, n, nullable, L, 0.01 if how == "limit" else 0.1, span) for k in kinds]  # limit: fewer NULLs than rows kept
        a = asc or [True, False, True][:len(kinds)]

        def fn(B, h):
            if how == "nulls":
                return [ordered([plain(B.sort_indices_nulls(h, a, [i % 2 == 1 for i in range(len(h))]))])]
            if how == "limit":
                return [ordered([plain(B.sort_indices_limit(h, a, 500))])]
            return [ordered([plain(B.sort_indices(h, a))])]
        return Case(cols, fn, env=env, ran=ran)


for _kind in ("int64", "int32", "float64"):
    for _nullable in (False, True):
        _s = "%s-%s" % (_kind, "null" if _nullable else "nn")
        add_sort("sort_indices-" + _s, [_kind], _nullable)
        add_sort("sort_indices-desc-" + _s, [_kind], _nullable, asc=[False])
        add_sort("sort_indices_nulls-" + _s, [_kind], _nullable, how="nulls", asc=[False])
        add_sort("sort_indices_limit-" + _s, [_kind], _nullable, how="limit")
        # the radix select (forced below its size threshold, as test_topk.py does), then the same with it off
        add_sort("sort_indices_limit-topk-" + _s, [_kind], _nullable, how="limit", env={"QEH_TOPK_MIN_ROWS": "0"},
                 ran=("topk_select",), span=10 ** 6)
        add_sort("sort_indices_limit-no_topk-" + _s, [_kind], _nullable, how="limit", env={"QEH_NO_TOPK": "1"}, span=10 ** 6)
for _nullable in (False, True):
    _s = "null" if _nullable else "nn"
    add_sort("sort_indices-pair-" + _s, ["int32", "int64"], _nullable, asc=[True, False])
    add_sort("sort_indices-no_pair-" + _s, ["int32", "int64"], _nullable, asc=[True, False], env={"QEH_NO_PAIR_SORT": "1"})
    add_sort("sort_indices_limit-topk-pair-" + _s, ["int64", "int32"], _nullable, how="limit", env={"QEH_TOPK_MIN_ROWS": "0"},
             ran=("topk_select",), asc=[True, False], span=40)
    add_sort("sort_indices-utf8_secondary-" + _s, ["int32", "utf8"], _nullable, asc=[False, True])
    add_sort("sort_indices_nulls-utf8_secondary-" + _s, ["int64", "utf8", "float64"], _nullable, how="nulls")


# ---- row_number / window --------------------------------------------------------------------------------
def add_window(name, func, param=0, default=None, msd=False, alias_arg=True, vkind="int64", two=False, nullable=False):
    """PARTITION BY k ORDER BY v [, u]; value functions take v itself (alias) or a third column."""
    @case(name)
    def build(lead):
        L, r = S.lead_cycle(lead), rng(name, lead)
        m = (lambda: mask(r, N)) if nullable else (lambda: None)
        k = make(ints(r, 0, 700, N) + 1000, m(), L(), key=True)
        v = make(ints(r, -40, 40, N) if vkind == "int64" else whole(r, N), m(), L(), key=vkind == "int64")
        cols = [k, v]
        if two:
            cols += [make(ints(r, 0, 5, N, I32), m(), L(), key=True), make(np.round(r.standard_normal(N), 1), m(), L())]
        value_fn = func in (WF.Lag, WF.Lead, WF.FirstValue, WF.LastValue)
        alias = alias_arg and not two  # two order keys: over ties of the first, FIRST_VALUE(v) never depends on the second
        if value_fn and not alias:
            cols.append(make(whole(r, N), m(), L()))

        def fn(B, h):
            part = [h[0]] + ([h[2]] if two else [])
            order = [h[1]] + ([h[3]] if two else [])
            asc = [False, True][:len(order)]
            if func == WF.RowNumber:
                return [ordered([plain(B.row_number(part, order, asc))])]
            arg = None if not value_fn else (h[1] if alias else h[-1])
            return [ordered([B.window(func, part, order, asc, arg=arg, param=param, default=default)])]
        env = {"QEH_WINDOW_MSD": "1"} if msd else None
        return Case(cols, fn, env=env, ran=("window_sort|w3_place",) if msd else ())


WINDOW_FUNCS = [("row_number", WF.RowNumber, 0, None), ("rank", WF.Rank, 0, None), ("dense_rank", WF.DenseRank, 0, None),
                ("ntile", WF.Ntile, 3, None), ("lag", WF.Lag, 1, None), ("lead", WF.Lead, 2, -5),
                ("first_value", WF.FirstValue, 0, None), ("last_value", WF.LastValue, 0, None)]
for _n, _f, _p, _d in WINDOW_FUNCS:
    add_window("window-%s" % _n, _f, _p, _d)
    add_window("window-%s-msd" % _n, _f, _p, _d, msd=True)
    add_window("window-%s-two_keys-null" % _n, _f, _p, None if _d is None else -5.0, two=True, nullable=True)
for _n, _f, _p, _d in WINDOW_FUNCS[4:]:
    add_window("window-%s-float64_order-msd" % _n, _f, _p, None if _d is None else -5.0, msd=True, vkind="float64")
    add_window("window-%s-own_argument-null" % _n, _f, _p, None if _d is None else -5.0, alias_arg=False, nullable=True)


# ---- partitioning and reordering ------------------------------------------------------------------------
def add_partition(name, how, kdt=I64, nullable=False):
    @case(name)
    def build(lead):
        L, r = S.lead_cycle(lead), rng(name, lead)
        if how == "range":
            from qe_hip.device import order_keys
            key = make(np.round(r.standard_normal(N), 2), mask(r, N) if nullable else None, L())
            split = np.sort(order_keys(np.array([-1.0, -0.0, 0.5, 1.25])))
            return Case([key], lambda B, h: [ordered([plain(x)]) for x in B.range_partition(h[0], split, False)])
        key = make(ints(r, 0, 5000, N, kdt), mask(r, N) if nullable else None, L(), key=True)
        return Case([key], lambda B, h: [ordered([plain(x)]) for x in B.hash_partition(h[0], 7)])


for _nullable in (False, True):
    _s = "null" if _nullable else "nn"
    add_partition("hash_partition-int64-" + _s, "hash", I64, _nullable)
    add_partition("hash_partition-int32-" + _s, "hash", I32, _nullable)
    add_partition("range_partition-float64-" + _s, "range", nullable=_nullable)


def add_partition_move(name, parts, kdt=I64, nullable=False, two_keys=False):
    @case(name)
    def build(lead):
        L, r = S.lead_cycle(lead), rng(name, lead)
        keys = [make(ints(r, -1000, 1000, N, kdt), mask(r, N) if nullable else None, L(), key=True)]
        if two_keys:
            keys.append(make(ints(r, 0, 9, N, I32), None, L(), key=True))
        cols = [make(whole(r, N), None, L()), make(ints(r, -10 ** 9, 10 ** 9, N), None, L()),
                make(ints(r, 0, 5, N), mask(r, N, 0.3), L()), make(r.random(N) > 0.5, mask(r, N), L()),
                make(np.array(["t%d" % (i % 11) * (i % 3) for i in range(N)], dtype=object), mask(r, N), L()),
                make(whole(r, N, F32), "buffer", L())]
        nk = len(keys)

        def fn(B, h):
            counts, moved = B.partition_hash_move(h[:nk], parts, h)
            return [ordered([plain(counts)]), ordered(moved)]
        return Case(keys + cols, fn)


add_partition_move("partition_hash_move-16parts", 16)
add_partition_move("partition_hash_move-256parts", 256)
add_partition_move("partition_hash_move-int32_key", 7, kdt=I32)
add_partition_move("partition_hash_move-null_key", 7, nullable=True)
add_partition_move("partition_hash_move-two_keys", 7, two_keys=True)


@case("partition_hash_unmove")
def _unmove(lead):
    """The key must be 16-B aligned (the entry point refuses others), so it takes leads 2 and 8 only;
    the moved columns, made by the reference's move, take every lead."""
    L, r = S.lead_cycle(lead), rng("partition_hash_unmove", lead)
    kv = ints(r, -(1 << 40), 1 << 40, N)
    key = make(kv, None, 2 if lead in (1, 2) else 8, key=True)
    _, moved = S.Host().partition_hash_move([(kv, None)], 8, [(whole(r, N), None), (np.arange(N, dtype=I64), None)])
    cols = [key, make(moved[0][0], None, L(), table=1), make(moved[1][0], None, L(), table=1)]
    return Case(cols, lambda B, h: [ordered(B.partition_hash_unmove(h[0], 8, h[1:]))])


def add_filter_partition_move(name, kdt, parts):
    @case(name)
    def build(lead):
        L, r = S.lead_cycle(lead), rng(name, lead)
        cols = [make(ints(r, 0, 100, N), None, L(), poison=[99, -(2 ** 63), 2 ** 63 - 1]),  # the row after the slice passes
                make(ints(r, -5000, 5000, N, kdt), None, L(), key=True),
                make(whole(r, N), None, L()), make(ints(r, -9, 9, N), None, L())]
        pred = binop(col(0), BinaryOp.Greater, lit(49)) & binop(col(3), BinaryOp.NotEqual, lit(0))

        def fn(B, h):
            counts, moved = B.filter_partition_hash_move(h, pred, 1, parts, [2, 3])
            return [ordered([plain(counts)]), ordered(moved)]
        return Case(cols, fn)


add_filter_partition_move("filter_partition_hash_move-int64-7parts", I64, 7)
add_filter_partition_move("filter_partition_hash_move-int64-40parts", I64, 40)
add_filter_partition_move("filter_partition_hash_move-int32-7parts", I32, 7)


def payload(r, kind, n, nullable, L, table=0):
    m = mask(r, n) if nullable else None
    if kind == "utf8":
        return make(np.array(["s%d" % x * (x % 4) for x in r.integers(0, 100, n)], dtype=object), m, L(), table=table)
    if kind == "bool":
        return make(r.random(n) > 0.5, m, L(), table=table)
    if kind == "int64":
        return make(ints(r, -(2 ** 62), 2 ** 62, n), m, L(), table=table)
    if kind == "int32":
        return make(ints(r, -1000, 1000, n, I32), m, L(), table=table)
    return make(whole(r, n, F64 if kind == "float64" else F32), m, L(), table=table)


GATHER_SRC = "a gather reads its source by row id, never by length"
for _kind in ("int64", "int32", "float64", "float32", "bool", "utf8"):
    for _nullable in (False, True):
        def _take(lead, kind=_kind, nullable=_nullable):
            name = "take-%s-%s" % (kind, nullable)
            L, r = S.lead_cycle(lead), rng(name, lead)
            src = payload(r, kind, N, nullable, L)
            idx = make(r.integers(0, N, 5003).astype(np.uint32), None, L(), inside=True, table=1)
            return Case([src, idx], lambda B, h: [ordered([B.take(h[0], h[1])])], exempt={("c", 0): GATHER_SRC})
        case("take-%s-%s" % (_kind, "null" if _nullable else "nn"))(_take)
for _kind in ("int64", "int32", "float64", "float32"):
    def _scatter(lead, kind=_kind):
        name = "scatter-%s" % kind
        L, r = S.lead_cycle(lead), rng(name, lead)
        src = payload(r, kind, N, False, L)
        perm = make(r.permutation(N).astype(np.uint32), None, L(), inside=True)
        return Case([src, perm], lambda B, h: [ordered([B.scatter(h[0], h[1])])])
    case("scatter-%s" % _kind)(_scatter)


CONCAT_SIZES = [1000, 0, 4097, 33]
for _kind in ("int64", "float32", "bool", "utf8"):
    for _nullable in (False, True):
        def _concat(lead, kind=_kind, nullable=_nullable):
            name = "concat-%s-%s" % (kind, nullable)
            L, r = S.lead_cycle(lead), rng(name, lead)
            parts = [payload(r, kind, n, nullable, L, table=t) for t, n in enumerate(CONCAT_SIZES) if n]
            return Case(parts, lambda B, h: [ordered([B.concat(h)])])
        case("concat-%s-%s" % (_kind, "null" if _nullable else "nn"))(_concat)


def add_merge_sorted(name, nullable):
    @case(name)
    def build(lead):
        L, r = S.lead_cycle(lead), rng(name, lead)
        kinds = ["int64", "float64", "bool", "utf8", "int32"]
        parts = []
        for t, n in enumerate((7001, 3333, 9)):
            p = [payload(r, k, n, nullable, L, table=t) for k in kinds]
            p[0] = make(ints(r, -300, 300, n), mask(r, n) if nullable else None, L(), table=t)
            parts.append(p)
        flat = [c for p in parts for c in p]
        w = len(kinds)

        def fn(B, h):
            return [ordered(B.merge_sorted([h[i * w:(i + 1) * w] for i in range(len(parts))], [0, 4], [False, True], [False, True]))]
        return Case(flat, fn)


def add_merge_payload(name, n, kdt, nullable, span, asc, nf, key_col=0, vdt=F64):
    """One sort key and one non-null 8-byte payload: the payload sort, whose first pass reads the
    partitions in place (keys through their column references, payloads at values + offset).  With
    2^20 rows or more and key codes of 24 to 45 bits it takes its MSD passes; the reference is then
    numpy's stable lexsort of the concatenation."""
    @case(name)
    def build(lead):
        L, r = S.lead_cycle(lead), rng(name, lead)
        sizes = [n // 2 + 1, 9, n - n // 2 - 10] if n < 2 ** 20 else [n - 9, 9]
        parts = []
        for t, m in enumerate(sizes):
            k = make(ints(r, -span, span, m, kdt), mask(r, m) if nullable else None, L(), table=t)
            v = make(whole(r, m) if vdt == F64 else ints(r, -(2 ** 62), 2 ** 62, m), None, L(), table=t)
            parts.append([k, v] if key_col == 0 else [v, k])
        flat = [c for p in parts for c in p]

        def fn(B, h):
            return [ordered(B.merge_sorted([h[2 * i:2 * i + 2] for i in range(len(parts))], [key_col], [asc], [nf], numpy=True))]
        return Case(flat, fn)


add_merge_payload("merge_sorted-payload-int64-nn", N, I64, False, 5000, True, True)
add_merge_payload("merge_sorted-payload-int64-null-desc_nulls_last", N, I64, True, 5000, False, False)
add_merge_payload("merge_sorted-payload-int32-null-key_second", N, I32, True, 100, True, True, key_col=1, vdt=I64)
add_merge_payload("merge_sorted-payload-msd-int64-nn", N_MSD_SORT, I64, False, 2 ** 29, True, True)
add_merge_payload("merge_sorted-payload-msd-int64-null", N_MSD_SORT, I64, True, 2 ** 29, True, False)
add_merge_sorted("merge_sorted-nn", False)
add_merge_sorted("merge_sorted-null", True)


# ---- other entry points --------------------------------------------------------------------------------
def add_avg_finalize(name, kind, sum_bitmap):
    @case(name)
    def build(lead):
        L, r = S.lead_cycle(lead), rng(name, lead)
        cnt = ints(r, 0, 10, N)
        if kind == "f64":
            s = make(ints(r, -1000, 1000, N).astype(F64) * 0.5, mask(r, N, 0.25) if sum_bitmap else None, L())
        else:  # Int32 input: the Int64 sums wrap to 32 bits first
            s = make(ints(r, -2 ** 33, 2 ** 33, N), mask(r, N, 0.25) if sum_bitmap else None, L())
        c = make(cnt, mask(r, N), L(), poison=[3, 5, 7])
        dt = abi.DT_FLOAT64 if kind == "f64" else abi.DT_INT32
        return Case([s, c], lambda B, h: [ordered([B.avg_finalize(h[0], h[1], dt)])], ran=("avg_finalize",))


for _kind in ("f64", "i32"):
    add_avg_finalize("avg_finalize-%s" % _kind, _kind, False)
    add_avg_finalize("avg_finalize-%s-null_sums" % _kind, _kind, True)


def add_in_set(name, kind, nullable, negated, env=None):
    @case(name)
    def build(lead):
        L, r = S.lead_cycle(lead), rng(name, lead)
        dom = np.arange(-300, 300)
        have = r.permutation(dom)[:200]
        lack = np.setdiff1d(dom, have)
        conv = (lambda a: np.array(["key%d" % x for x in a], dtype=object)) if kind == "utf8" else (lambda a: np.asarray(a, I32))
        probe = make(conv(r.choice(dom, N)), mask(r, N) if nullable else None, L(), key=kind != "utf8")
        # rows next to the set's slice: keys the set lacks (they would turn misses into hits)
        sset = make(conv(have), mask(r, len(have), 0.02, last=False) if nullable else None, L(), table=1, poison=conv(lack[:3]))
        return Case([probe, sset], lambda B, h: [ordered([B.in_set(h[0], h[1], negated)])], env=env)


for _kind in ("int32", "utf8"):
    for _nullable in (False, True):
        for _neg in (False, True):
            add_in_set("in_set-%s-%s%s" % (_kind, "null" if _nullable else "nn", "-not" if _neg else ""), _kind, _nullable, _neg)
add_in_set("in_set-int32-nn-hash_form", "int32", False, False, env={"QEH_IN_SET": "hash"})
add_in_set("in_set-int32-null-bitmap_form", "int32", True, True, env={"QEH_IN_SET": "bitmap"})


def add_eval(name, kinds, nullable, expr):
    @case(name)
    def build(lead):
        L, r = S.lead_cycle(lead), rng(name, lead)
        m = (lambda: mask(r, N)) if nullable else (lambda: None)
        gen = {"int64": lambda: make(ints(r, -1000, 1000, N), m(), L(), key=True), "float64": lambda: make(whole(r, N), m(), L()),
               "int32": lambda: make(ints(r, -100, 100, N, I32), m(), L(), key=True), "bool": lambda: make(r.random(N) > 0.5, m(), L())}
        return Case([gen[k]() for k in kinds], lambda B, h: [ordered([B.eval(h, expr)])])


def arith(c):
    return binop(binop(col(0), BinaryOp.Multiply, c), BinaryOp.Add, binop(col(1), BinaryOp.Subtract, col(0)))


BOOLEX = (binop(col(0), BinaryOp.Greater, col(1)) & UnaryExpr(UnaryOp.Not, col(2))) | binop(col(3), BinaryOp.LessEqual, lit(-10.0))
for _nullable in (False, True):
    _s = "null" if _nullable else "nn"
    add_eval("eval-arithmetic-int64-" + _s, ["int64", "int64"], _nullable, arith(lit(3)))
    add_eval("eval-arithmetic-float64-" + _s, ["float64", "float64"], _nullable, arith(lit(3.0)))
    add_eval("eval-arithmetic-int32-" + _s, ["int32", "int32"], _nullable, binop(col(0), BinaryOp.Add, col(1)))
    add_eval("eval-bool-" + _s, ["int64", "int64", "bool", "float64"], _nullable, BOOLEX)


def add_encode(name, how, nullable):
    @case(name)
    def build(lead):
        L, r = S.lead_cycle(lead), rng(name, lead)
        n = 5003
        kinds = ["int64", "int32", "float64", "float32", "bool", "utf8"]
        cols = [payload(r, k, n, nullable, L) for k in kinds]
        if how == "pg":
            return Case(cols, lambda B, h: [ordered([B.encode_pg_datarows(h)])])
        return Case(cols, lambda B, h: [ordered(B.encode_arrow_ipc(h, ["g." + k for k in kinds]))])


for _nullable in (False, True):
    _s = "null" if _nullable else "nn"
    add_encode("encode_pg_datarows-" + _s, "pg", _nullable)
    add_encode("encode_arrow_ipc-" + _s, "ipc", _nullable)


def add_filter(name, nullable, env=None, max_rows=None):
    @case(name)
    def build(lead):
        L, r = S.lead_cycle(lead), rng(name, lead)
        m = (lambda: mask(r, N, last=False)) if nullable else (lambda: None)
        x, b = ints(r, 0, 100, N), r.random(N) > 0.5
        x[0], b[0], b[-S.TRAIL] = 99, True, False  # the first row and the row after the slice qualify
        cols = [make(x, m(), L(), poison=[99, -(2 ** 63), 2 ** 63 - 1]), make(b, m(), L())] + \
               [payload(r, k, N, nullable, L) for k in ("int64", "int32", "float64", "float32", "utf8")]
        pred = binop(col(0), BinaryOp.Greater, lit(49)) & col(1)
        return Case(cols, lambda B, h: [ordered(B.filter(h, pred, list(range(len(h))), max_rows))], env=env)


for _nullable in (False, True):
    _s = "null" if _nullable else "nn"
    add_filter("filter-" + _s, _nullable)
    add_filter("filter-no_fast-" + _s, _nullable, env={"QEH_NO_FAST_FILTER": "1"})
    add_filter("filter_limit-" + _s, _nullable, max_rows=N // 2 + 3000)  # more rows than qualify without the row after the slice


def add_fast_filter(name, nterms):
    """non-null 8-byte columns and column-literal terms: the fast filter's shape"""
    @case(name)
    def build(lead):
        L, r = S.lead_cycle(lead), rng(name, lead)
        cols = [make(ints(r, 0, 100, N), None, L(), poison=[99, -(2 ** 63), 2 ** 63 - 1]), make(whole(r, N), None, L(), poison=[-7.0, np.nan]),
                make(ints(r, -(2 ** 62), 2 ** 62, N), None, L())]
        pred = binop(col(0), BinaryOp.Greater, lit(49))
        if nterms == 2:
            pred = pred & binop(col(1), BinaryOp.Less, lit(10.0))
        ex = {("a", 1): "the one-term predicate does not name it, and it is not an output"} if nterms == 1 else {}
        return Case(cols, lambda B, h: [ordered(B.filter(h, pred, [0, 2] if nterms == 1 else [0, 1, 2]))], exempt=ex)


add_fast_filter("filter-fast-1term", 1)
add_fast_filter("filter-fast-2terms", 2)


@case("columns_minmax")
def _minmax(lead):
    L, r = S.lead_cycle(lead), rng("columns_minmax", lead)
    cols = [make(ints(r, -10 ** 9, 10 ** 9, N), None, L()), make(ints(r, -1000, 1000, N, I32), mask(r, N), L()),
            make(ints(r, 5, 900, N), mask(r, N, 0.5), L())]
    return Case(cols, lambda B, h: [ordered([plain(B.columns_minmax(h).ravel())])])


def add_utf8(name, how, nullable, jt="inner"):
    @case(name)
    def build(lead):
        L, r = S.lead_cycle(lead), rng(name, lead)
        words = np.array(["w%03d" % i * (1 + i % 3) for i in range(400)], dtype=object)
        if how == "dict":
            c = make(words[r.integers(0, 300, N)], mask(r, N) if nullable else None, L())
            return Case([c], lambda B, h: [ordered([x]) for x in B.utf8_dict_encode(h[0])])
        nb = 2000
        bk = make(words[r.integers(0, 300, nb)], mask(r, nb, last=False) if nullable else None, L(), table=1, poison=words[300:303])
        pk = make(words[r.integers(0, 400, N)], mask(r, N, 0.05, last=False) if nullable else None, L(), poison=words[:3])
        cols = [pk, make(np.arange(N, dtype=I64) * 7, None, L()), bk, make(np.arange(nb, dtype=I64) * 3 + (1 << 40), None, L(), table=1)]
        return Case(cols, lambda B, h: [multiset(B.join_utf8(JT[jt], h[0], [h[1]], h[2], [h[3]]))])


for _nullable in (False, True):
    _s = "null" if _nullable else "nn"
    add_utf8("utf8_dict_encode-" + _s, "dict", _nullable)
    for _jt in ("inner", "left", "right", "full"):
        add_utf8("hash_join-utf8_keys-%s-%s" % (_jt, _s), "join", _nullable, _jt)


# ---- the tests ---------------------------------------------------------------------------------------------
def readings(c):
    """(label, {column: mode}) of every wrong reading of the case's parents"""
    for j, colj in enumerate(c.cols):
        yield ("a", j), {j: "a"}
        if colj.pvalid is not None:
            yield ("b", j), {j: "b"}
    for t in sorted({x.table for x in c.cols}):
        yield ("c", t), {j: "c" for j, x in enumerate(c.cols) if x.table == t}


@pytest.mark.parametrize("lead", S.LEADS)
@pytest.mark.parametrize("name", list(CASES))
def test_inputs_discriminate(name, lead):
    c = CASES[name](lead)
    B = S.Host()
    want = c.fn(B, [B.col(x) for x in c.cols])
    leads = {x.lead for x in c.cols}
    assert len(c.cols) < 2 or len(leads) > 1, "the columns of one call take different leads"
    exempt = c.exempt
    same = []
    for label, modes in readings(c):
        if label in exempt:
            continue
        try:
            got = c.fn(B, [B.col(x, modes.get(j, "ok")) for j, x in enumerate(c.cols)])
        except (ob.OracleError, ValueError, IndexError):
            continue  # the reference refuses the misread input outright: a different answer
        if not any(g != w for g, w in zip(got, want)):
            same.append(label)
    assert not same, "readings that do not change the answer of %s: %s" % (name, same)


def run_on_device(ctx, monkeypatch, c, aligned):
    for k, v in c.env.items():
        monkeypatch.setenv(k, v)
    B = S.Dev(ctx)
    h = [B.col(x) for x in c.cols]
    for x, d in zip(c.cols, h):
        assert d.c.offset == x.lead and d.c.null_count == (-1 if x.pvalid is not None else 0)
    ctx.timing(True)
    ctx.timing_reset()
    try:
        got = c.fn(B, h)
        if aligned:
            for rec in c.ran:
                assert any(ctx.kernel_time(x)[1] >= 1 for x in rec.split("|")), "the forced path did not run: " + rec
            for rec in c.absent:
                assert ctx.kernel_time(rec)[1] == 0, "another path ran: " + rec
    finally:
        ctx.timing(False)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("lead", S.LEADS)
@pytest.mark.parametrize("name", list(CASES))
def test_sliced_matches_reference(ctx, monkeypatch, name, lead):
    c = CASES[name](lead)
    H = S.Host()
    want = c.fn(H, [H.col(x) for x in c.cols])
    got = run_on_device(ctx, monkeypatch, c, aligned=lead in (2, 8))
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s lead %d result %d: %s" % (name, lead, i, g.diff(w))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["join-left-narrow_records_dup_null_build_keys", "join-right-narrow_records_dup_null_build_keys",
                                  "join-full-narrow_records_dup_null_build_keys"])
def test_narrow_records_fallback_unsliced(ctx, name):
    """The duplicate-key fallback out of the prebuilt records, on plain (offset 0) columns."""
    c = CASES[name](1)
    H, B = S.Host(), S.Dev(ctx, sliced=False)
    want = c.fn(H, [H.col(x) for x in c.cols])
    got = c.fn(B, [B.col(x) for x in c.cols])
    assert got[0] == want[0], got[0].diff(want[0])


# ---- plans: Limit's zero-copy views under another operator ------------------------------------------------
# SELECT ... FROM (SELECT * FROM t LIMIT fetch OFFSET skip) ...: the executor's Limit hands views with
# offset += skip (and an unknown NULL count) to the operator above it.  Reference: the oracle on
# t.slice(skip, fetch) of the host table.
SKIPS = (1, 8, 67)
PLAN_ROWS = 20_011


@pytest.fixture(scope="module")
def qx(ctx):
    from qe_hip import QueryExecutor
    return QueryExecutor(ctx)


@pytest.fixture(scope="module")
def tables():
    import pyarrow as pa
    r = np.random.default_rng(0x51CE)
    n = PLAN_ROWS
    t = pa.table({"t.k": pa.array(ints(r, 0, 40, n), pa.int64(), mask=r.random(n) < 0.05),
                  "t.v": pa.array(ints(r, -100, 100, n), pa.int64()),
                  "t.w": pa.array(whole(r, n), pa.float64(), mask=r.random(n) < 0.1),
                  "t.x": pa.array(ints(r, 0, 100, n), pa.int64())})
    nd = 3000
    d = pa.table({"d.k": pa.array(ints(r, 0, 60, nd), pa.int64(), mask=r.random(nd) < 0.05),
                  "d.a": pa.array(ints(r, -9, 9, nd), pa.int32())})
    return t, d


def limited(table, skip, tail=200):
    """(the Limit plan over the table's scan, the host columns of the same rows)"""
    from qe_hip import Limit, Scan
    from test_executor import as_cols, source
    fetch = table.num_rows - skip - tail
    host = as_cols(table.slice(skip, fetch).combine_chunks().to_batches())
    return Limit(Scan(source(table)), skip, fetch), host


def plan_cols(batches):
    from test_executor import as_cols
    return as_cols(batches)


@pytest.mark.gpu
@pytest.mark.parametrize("skip", SKIPS)
def test_plan_sort_over_limit(qx, tables, skip):
    from qe_hip import Sort
    from qe_hip.expr import Column
    plan, host = limited(tables[0], skip)
    got = plan_cols(qx.execute(Sort(plan, [Column("t.k", 0), Column("t.w", 2)], [True, False])))
    perm = ob.sort_indices([ob.HostCol(*host[0]), ob.HostCol(*host[2])], [True, False]).astype(I64)
    want = [(v[perm], m[perm]) for v, m in host]
    assert ordered(got) == ordered(want), ordered(got).diff(ordered(want))


@pytest.mark.gpu
@pytest.mark.parametrize("asc", [True, False])
@pytest.mark.parametrize("skip", SKIPS)
def test_plan_key_payload_sort_over_limit(qx, tables, skip, asc):
    """A two-column table sorted by its Int key: the payload rides through the radix passes."""
    from qe_hip import Sort
    from qe_hip.expr import Column
    plan, host = limited(tables[0].select(["t.k", "t.w"]).set_column(1, "t.w", tables[0].column("t.v").cast("float64")), skip)
    got = plan_cols(qx.execute(Sort(plan, [Column("t.k", 0)], [asc])))
    perm = ob.sort_indices([ob.HostCol(*host[0])], [asc]).astype(I64)
    want = [(v[perm], m[perm]) for v, m in host]
    assert ordered(got) == ordered(want), ordered(got).diff(ordered(want))


PLAN_AGGS = [(AF.Sum, 1), (AF.Count, 2), (AF.Sum, 2), (AF.Min, 2), (AF.Max, 1), (AF.Count, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("skip", SKIPS)
def test_plan_aggregate_over_limit(qx, tables, skip, filtered):
    from qe_hip import AggregateExpr, Filter, HashAggregate
    from qe_hip.expr import Column
    plan, host = limited(tables[0], skip)
    names = ["t.k", "t.v", "t.w", "t.x"]
    pred = binop(Column("t.x", 3), BinaryOp.Greater, lit(49))
    if filtered:
        plan = Filter(plan, pred)
    got = plan_cols(qx.execute(HashAggregate(plan, [Column("t.k", 0)], [AggregateExpr(f, Column(names[c], c)) for f, c in PLAN_AGGS])))
    wk, wa = S.Host().filter_aggregate(host, pred if filtered else None, [0], PLAN_AGGS)
    assert multiset(got) == multiset(wk + wa), multiset(got).diff(multiset(wk + wa))


@pytest.mark.gpu
@pytest.mark.parametrize("func,param", [(WF.RowNumber, 0), (WF.Rank, 0), (WF.Lag, 1)])
@pytest.mark.parametrize("skip", SKIPS)
def test_plan_window_over_limit(qx, tables, skip, func, param):
    from qe_hip import Window, WindowExpr
    from qe_hip.expr import Column
    plan, host = limited(tables[0], skip)
    value_fn = func == WF.Lag
    args = [Column("t.w", 2)] + ([lit(param)] if param else []) if value_fn else []
    win = Window(plan, [WindowExpr(func, args, [Column("t.k", 0)], [Column("t.v", 1)])], ["t.k", "t.v", "t.w", "t.x", "f"])
    got = plan_cols(qx.execute(win))
    H = S.Host()
    if func == WF.RowNumber:
        want = plain(H.row_number([host[0]], [host[1]], [True]))
    else:
        want = H.window(func, [host[0]], [host[1]], [True], arg=host[2] if value_fn else None, param=param)
    assert ordered(got[:4]) == ordered(host)  # the input columns pass through
    assert ordered(got[4:]) == ordered([want]), ordered(got[4:]).diff(ordered([want]))


@pytest.mark.gpu
@pytest.mark.parametrize("jt", ["inner", "left", "full"])
@pytest.mark.parametrize("skip", SKIPS)
def test_plan_join_over_limits(qx, tables, skip, jt):
    from qe_hip import HashJoin, JoinType
    from qe_hip.expr import Column
    left, lhost = limited(tables[0], skip)
    right, rhost = limited(tables[1], {1: 67, 8: 1, 67: 8}[skip])  # the two sides take different offsets
    kind = {"inner": JoinType.Inner, "left": JoinType.Left, "full": JoinType.Full}[jt]
    got = plan_cols(qx.execute(HashJoin(left, right, kind, binop(Column("t.k", 0), BinaryOp.Equal, Column("d.k", 4)))))
    H = S.Host()
    want = H.join_inner(lhost[0], lhost, rhost[0], rhost) if jt == "inner" else H.join_outer(JT[jt], lhost[0], lhost, rhost[0], rhost)
    assert multiset(got) == multiset(want), multiset(got).diff(multiset(want))


@pytest.mark.gpu
@pytest.mark.parametrize("negated", [False, True])
@pytest.mark.parametrize("skip", SKIPS)
def test_plan_in_subquery_over_limit(qx, tables, skip, negated):
    """t.x [NOT] IN (SELECT a FROM (SELECT * FROM d LIMIT .. OFFSET skip)): the set is a sliced column."""
    import pyarrow as pa
    from qe_hip import Filter, InSubquery, Projection, Scan
    from test_executor import as_cols, source
    t = tables[0]
    d = pa.table({"d.a": pa.array(np.arange(200, dtype=I64))})  # the rows cut off at either end change the set: skip .. 79
    sub, shost = limited(d, skip, tail=120)
    plan = Filter(Scan(source(t)), InSubquery(col(3), Projection(sub, [col(0)], ["a"]), negated=negated))
    got = plan_cols(qx.execute(plan))
    host = as_cols(t.combine_chunks().to_batches())
    keep = np.isin(host[3][0], shost[0][0]) != negated
    want = [(v[keep], m[keep]) for v, m in host]
    assert 0 < keep.sum() < len(keep)
    assert ordered(got) == ordered(want), ordered(got).diff(ordered(want))
