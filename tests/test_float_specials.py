"""Float special values (signed zeros, subnormals, infinities, NaNs of both signs and several
payloads) through every operator that compares, orders, groups or aggregates floats.

The contract is IEEE totalOrder (arrow-rs `total_cmp`): -0.0 < +0.0 and the two are different
group keys; a positive NaN is above +inf and equal only to the same bits; a negative NaN is below
-inf; values pass through operators bit for bit.

CPU half: the oracle against a NumPy restatement written on the integer view of the bits
(specials.total_key).  GPU half: the device against the oracle, and against NumPy where that is
cheap, by bit pattern and validity.  The only results not compared by bits are NaNs that
arithmetic or a SUM / AVG produced or carried (isnan_only): x86 and the GPU give the default NaN
different signs and the payload a sum carries depends on the order of the additions.

Every GPU case either checks the KernelTimer launch count of the path it aims at or runs under
both settings of that path's environment toggle and requires the same bits from both."""
import math

import numpy as np
import pytest

import oracle_bind as ob
from qe_hip import AggregateFunction as AF
from qe_hip import BinaryOp, ScalarValue, UnaryExpr, UnaryOp, binop, col, lit
from qe_hip.expr import Literal
from qe_hip.plan import WindowFunctionType as W
from specials import (F32_SPECIALS, F64_SPECIALS, TILE, assert_bits_equal, assert_grouped_bits_equal, bits_of,
                      exact_summable, f64, special_positions, specials_of, total_key, with_specials)

N_TAIL = TILE + 1          # a full tile and a one-row ragged tail
N_MULTI = 3 * TILE + 5     # several tiles, more than one workgroup's worth
SIZES = [1, N_TAIL, N_MULTI]

POS_NAN, NEG_NAN = f64(0x7FF8000000000000), f64(0xFFF8000000000000)
MAX_NAN, MIN_NAN = f64(0x7FFFFFFFFFFFFFFF), f64(0xFFFFFFFFFFFFFFFF)  # order keys INT64_MAX / INT64_MIN
SUB = 5e-324

OPS = {
    "eq": (BinaryOp.Equal, np.equal), "ne": (BinaryOp.NotEqual, np.not_equal),
    "lt": (BinaryOp.Less, np.less), "le": (BinaryOp.LessEqual, np.less_equal),
    "gt": (BinaryOp.Greater, np.greater), "ge": (BinaryOp.GreaterEqual, np.greater_equal),
}


def rng(*seed):
    return np.random.default_rng([int(s) for s in seed])


def wide_floats(r, n, dtype):
    """standard_normal * 10**randint over most of the type's exponent range"""
    span = 300 if np.dtype(dtype) == np.float64 else 30
    with np.errstate(over="ignore", under="ignore"):
        return (r.standard_normal(n) * 10.0 ** r.integers(-span, span, n)).astype(dtype)


def laden(n, dtype, *seed, every=2, nulls=False):
    """(values, validity): half the rows (every=2) are specials, first lane pair, last row and both
    sides of every tile boundary among them; 10 % NULLs when asked."""
    r = rng(n, *seed)
    v = with_specials(wide_floats(r, n, dtype), specials_of(dtype), r, every)
    return v, ((r.random(n) > 0.1) if nulls else None)


def valid_of(c):
    return np.ones(len(c[0]), bool) if c[1] is None else np.asarray(c[1], bool)


def host(cols):
    return [ob.HostCol(v, m) for v, m in cols]


def test_with_specials_places_what_it_promises():
    for dt, sp in ((np.float64, F64_SPECIALS), (np.float32, F32_SPECIALS)):
        v, _ = laden(N_MULTI, dt, 0)
        hit = np.isin(bits_of(v), bits_of(sp))
        for row in (0, 1, N_MULTI - 1, TILE - 1, TILE, 2 * TILE - 1, 2 * TILE, 3 * TILE - 1, 3 * TILE):
            assert hit[row], row
        counts = [(bits_of(v) == b).sum() for b in bits_of(sp)]
        assert min(counts) >= 100  # each special many times
        assert 0.4 < hit.mean() < 0.6
    assert len(special_positions(1, rng(0), 2)) == 1
    k = total_key(F64_SPECIALS)
    assert k[16] == np.iinfo(np.int64).min and k[15] == np.iinfo(np.int64).max  # MIN_NAN, MAX_NAN
    assert k[1] == -1 and k[0] == 0  # -0.0 just below +0.0
    assert len(set(k.tolist())) == len(k) == len(set(total_key(F32_SPECIALS).tolist()))


def test_exact_summable_is_exact_in_any_order():
    x = exact_summable(rng(1), 2 ** 16)
    want = math.fsum(x.tolist())
    for perm_seed in range(3):
        assert float(np.add.reduce(rng(perm_seed).permutation(x))) == want
    assert float(x.cumsum()[-1]) == want  # sequential, no pairwise tree


# ---- predicates ------------------------------------------------------------------------------
# columns: 0 a f64, 1 b f64, 2 c int64 around +-(2**53 + 1), 3 f f32, 4 t bool (all true, never NULL)
F64_LITS = [-0.0, 0.0, np.inf, -np.inf, POS_NAN, MIN_NAN, MAX_NAN, SUB, 1.0]
INT_LITS = [-0.0, 2.0 ** 53, -(2.0 ** 53), np.inf, POS_NAN, NEG_NAN]


def pred_table(n, nulls, seed=0):
    r = rng(n, seed, 99)
    c = r.integers(-3, 4, n).astype(np.int64)
    big = np.array([2 ** 53 + 1, -(2 ** 53 + 1), 2 ** 53, -(2 ** 53), 2 ** 53 + 2, 0], np.int64)
    pos = special_positions(n, r, 3)
    c[pos] = big[np.arange(len(pos)) % len(big)]
    return [laden(n, np.float64, seed, 1, nulls=nulls), laden(n, np.float64, seed, 2, nulls=nulls),
            (c, (r.random(n) > 0.1) if nulls else None), laden(n, np.float32, seed, 3, nulls=nulls),
            (np.ones(n, bool), None)]


def operand_key(cols, x):
    """(order keys, validity) of a predicate operand: a column index or a float literal"""
    n = len(cols[0][0])
    if isinstance(x, int):
        v, _ = cols[x]
        return total_key(v if v.dtype.kind == "f" else v.astype(np.float64)), valid_of(cols[x])
    return np.full(n, total_key(np.array([x], np.float64))[0]), np.ones(n, bool)


def np_term(cols, a, op, b):
    """(truth, validity) of `a op b` by totalOrder; ints compared to a float go through Float64"""
    ka, va = operand_key(cols, a)
    kb, vb = operand_key(cols, b)
    return OPS[op][1](ka, kb), va & vb


def expr_term(a, op, b):
    def e(x):
        return col(x) if isinstance(x, int) else lit(float(x))
    return binop(e(a), OPS[op][0], e(b))


def np_rows(cols, keep, out_idx=None):
    out_idx = range(len(cols)) if out_idx is None else out_idx
    return [(cols[j][0][keep], valid_of(cols[j])[keep]) for j in out_idx]


def term_cases(op):
    """(name, left operand, right operand) of the predicate matrix for one compare op"""
    cases = [(f"f64 col {op} {x!r}", 0, x) for x in F64_LITS]
    cases += [(f"int64 col {op} {x!r}", 2, x) for x in INT_LITS]
    cases += [(f"f32 col {op} f64 col", 3, 0), (f"f64 col {op} f64 col", 0, 1)]
    return cases


@pytest.mark.parametrize("op", sorted(OPS))
def test_oracle_filter_matches_numpy(op):
    for n in SIZES:
        cols = pred_table(n, nulls=True)
        for name, a, b in term_cases(op):
            truth, valid = np_term(cols, a, op, b)
            keep = truth & valid
            want = np_rows(cols, keep)
            got, rows, _ = ob.filter(host(cols), expr_term(a, op, b))
            assert rows == keep.sum(), (name, n)
            for j in range(len(cols)):
                assert_bits_equal(got[j], want[j], f"{name} n={n} col {j}")
    # the matrix separates the operators: at the largest size no two of them keep the same rows
    # of `a op -0.0`, and both zeros, both NaN signs and both infinities are among the rows
    cols = pred_table(N_MULTI, nulls=True)
    t = np_term(cols, 0, op, -0.0)[0]
    others = [np_term(cols, 0, o, -0.0)[0] for o in OPS if o != op]
    assert all((t != o).any() for o in others)


# ---- sort order ------------------------------------------------------------------------------
def np_sort_perm(keys, asc, nulls_first):
    """stable lexicographic order by totalOrder keys; ~k reverses an Int64 order without overflow"""
    n = len(keys[0][0])
    cols = [np.arange(n)]
    for (v, m), a, nf in reversed(list(zip(keys, asc, nulls_first))):
        m = valid_of((v, m))
        k = total_key(v)
        cols.append(np.where(m, k if a else ~k, 0))
        cols.append(m if nf else ~m)
    return np.lexsort(cols).astype(np.uint32)


SORT_MODES = [(True, True), (True, False), (False, True), (False, False)]  # (ascending, nulls first)


def sort_keys(n, dt, nulls, seed=0):
    r = rng(n, seed, 7)
    return [laden(n, dt, seed, 11, nulls=nulls), (r.integers(-3, 3, n).astype(np.int64), None)]


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_oracle_sort_matches_numpy(dt):
    for n in [1, 7, N_TAIL, N_MULTI]:
        keys = sort_keys(n, dt, nulls=True)
        for asc, nf in SORT_MODES:
            got = ob.sort_indices_nulls(host(keys[:1]), [asc], [nf])
            assert np.array_equal(got, np_sort_perm(keys[:1], [asc], [nf])), (n, asc, nf)
            got = ob.sort_indices_nulls(host(keys), [asc, not asc], [nf, True])
            assert np.array_equal(got, np_sort_perm(keys, [asc, not asc], [nf, True])), (n, asc, nf)
        for asc in (True, False):  # qo_sort_indices: NULLs first either way
            got = ob.sort_indices(host(keys[:1]), [asc])
            assert np.array_equal(got, np_sort_perm(keys[:1], [asc], [True])), (n, asc)


# ---- aggregates ------------------------------------------------------------------------------
def designed_values(n, dt, gid, seed):
    """Values whose MIN / MAX per group id are, in turn: the two zeros; a negative NaN; the
    positive NaN with the largest payload; the all-ones NaN (Float64 order key INT64_MIN: the
    MIN / MAX initial state and the group table's empty marker); a subnormal MIN; +inf; -inf with
    a negative subnormal MAX; NULL (group 7); one repeated all-ones NaN; one repeated largest NaN.  Groups from 10 on draw from a
    special-laden column."""
    sp = specials_of(dt)
    z, nz, sub, nsub, mn, nmn, one, none_, mx, nmx, inf, ninf, qn, nqn, qn1, maxn, minn = sp
    sets = [[z, nz], [nqn, ninf, one], [maxn, qn, inf, one], [minn, nqn, ninf, z],
            [sub, mn, one], [inf, mx, none_], [ninf, nmn, nsub], [one], [minn], [maxn]]
    r = rng(n, seed, 5)
    v, _ = laden(n, dt, seed, 21)
    m = r.random(n) > 0.1
    for g, s in enumerate(sets):
        rows = np.flatnonzero(gid == g)
        v[rows] = np.array(s, dt)[r.integers(0, len(s), len(rows))]
    m[gid == 7] = False
    return v, m


def agg_table(n, groups, seed=0, nulls=True):
    """0 g int64 group id, 1 v f64 designed, 2 x f64 exact_summable, 3 w f32 designed, 4 h int64 (0..2)"""
    r = rng(n, groups, seed)
    gid = r.integers(0, groups, n).astype(np.int64)
    gid[:min(n, groups)] = np.arange(min(n, groups))  # every group present
    v, vm = designed_values(n, np.float64, gid, seed)
    w, wm = designed_values(n, np.float32, gid, seed + 1)
    x = exact_summable(r, n)
    xm = r.random(n) > 0.1
    gm = r.random(n) > 0.05
    if not nulls:
        return [(gid, None), (v, None), (x, None), (w, None), (r.integers(0, 3, n).astype(np.int64), None)]
    return [(gid, gm), (v, vm), (x, xm), (w, wm), (r.integers(0, 3, n).astype(np.int64), None)]


MINMAX_AGGS = [(AF.Min, 1), (AF.Max, 1), (AF.Count, 1), (AF.Min, 3), (AF.Max, 3), (AF.Count, 3), (AF.Count, 0)]
SUM_AGGS = [(AF.Sum, 2), (AF.Avg, 2), (AF.Count, 2)]


def np_group_ids(keys):
    """(group id per row, representative row per group): rows grouped by validity and bits of every key"""
    n = len(keys[0][0])
    parts = []
    for v, m in keys:
        m = valid_of((v, m))
        parts += [m.astype(np.int64), np.where(m, bits_of(v).astype(np.int64), 0)]
    rows = np.stack(parts, 1) if parts else np.zeros((n, 1), np.int64)
    _, rep, inv = np.unique(rows, axis=0, return_index=True, return_inverse=True)
    return inv.reshape(-1), rep


def np_min_max_count(keys, val):
    """per group (in np_group_ids order): MIN and MAX by totalOrder with their validity, and COUNT"""
    gid, rep = np_group_ids(keys)
    G = len(rep)
    v, m = val[0], valid_of(val)
    k = total_key(v)
    cnt = np.bincount(gid, weights=m, minlength=G).astype(np.int64)
    lo = np.lexsort((k, ~m, gid))  # valid rows first inside a group, then ascending key
    first = np.searchsorted(gid[lo], np.arange(G))
    hi = np.lexsort((~k, ~m, gid))
    return (v[lo][first], cnt > 0), (v[hi][first], cnt > 0), (cnt, np.ones(G, bool)), gid, rep


def np_group_keys(keys, rep):
    return [(v[rep], valid_of((v, m))[rep]) for v, m in keys]


@pytest.mark.parametrize("kdt", [np.int64, np.float64, np.float32])
def test_oracle_min_max_count_matches_numpy(kdt):
    n = N_MULTI
    cols = agg_table(n, 16)
    if kdt != np.int64:  # float keys: every special several times, and NULLs
        r = rng(3)
        cols[0] = (specials_of(kdt)[r.integers(0, 17, n)], r.random(n) > 0.05)
    keys = [cols[0]]
    wk, wa, wg, _ = ob.hash_aggregate(host(keys), host(cols), MINMAX_AGGS)
    mn64, mx64, c64, gid, rep = np_min_max_count(keys, cols[1])
    mn32, mx32, c32, _, _ = np_min_max_count(keys, cols[3])
    rows = np_min_max_count(keys, cols[0])[2]  # COUNT(key): 0 for the NULL group
    assert wg == len(rep) == (16 if kdt == np.int64 else 17) + 1  # the NULL group is its own
    assert_grouped_bits_equal(wk, wa, np_group_keys(keys, rep), [mn64, mx64, c64, mn32, mx32, c32, rows])
    if kdt == np.int64:  # the designed answers, so the cases above are really in the data
        by = {int(k): i for i, (k, ok) in enumerate(zip(wk[0][0], wk[0][1])) if ok}
        bits = lambda a, g: int(bits_of(wa[a][0])[by[g]]) & (2 ** 64 - 1)
        assert (bits(0, 0), bits(1, 0)) == (0x8000000000000000, 0)          # MIN -0.0, MAX +0.0
        assert bits(0, 1) == 0xFFF8000000000000 and bits(1, 2) == 0x7FFFFFFFFFFFFFFF
        assert bits(0, 3) == 0xFFFFFFFFFFFFFFFF and bits(0, 4) == 0x0000000000000001
        assert bits(1, 5) == 0x7FF0000000000000 and bits(0, 6) == 0xFFF0000000000000 and bits(1, 6) == 0x8000000000000001
        assert not wa[0][1][by[7]] and not wa[1][1][by[7]] and wa[2][0][by[7]] == 0
        assert bits(0, 8) == bits(1, 8) == 0xFFFFFFFFFFFFFFFF and bits(0, 9) == bits(1, 9) == 0x7FFFFFFFFFFFFFFF


@pytest.mark.parametrize("groups", [7, 1000])
def test_oracle_sum_avg_of_exact_summable_matches_fsum(groups):
    cols = agg_table(N_MULTI, groups)
    wk, wa, wg, _ = ob.hash_aggregate(host(cols[:1]), host(cols), SUM_AGGS)
    gid, rep = np_group_ids(cols[:1])
    x, xm = cols[2]
    sums, avgs, cnts = [], [], []
    for g in range(len(rep)):
        vals = x[(gid == g) & xm].tolist()
        cnts.append(len(vals))
        sums.append(math.fsum(vals))
        avgs.append(sums[-1] / len(vals) if vals else 0.0)  # one correctly rounded division
    some = np.array(cnts) > 0
    want = [(np.array(sums), some), (np.array(avgs), some), (np.array(cnts, np.int64), np.ones(len(rep), bool))]
    assert wg == len(rep) == groups + 1
    assert_grouped_bits_equal(wk, wa, np_group_keys(cols[:1], rep), want)


# ============================== GPU half ==========================================================
def timed(ctx, fn):
    """fn() with kernel timing on; returns (result, launch count by label)"""
    ctx.timing(True)
    ctx.timing_reset()
    try:
        out = fn()
        return out, lambda label: ctx.kernel_time(label)[1]
    finally:
        ctx.timing(False)


def dev_filter(ctx, cols, pred, out_idx=None):
    dev = [ctx.upload(v, m) for v, m in cols]
    (out, rows), launches = timed(ctx, lambda: ctx.filter(dev, pred, out_idx))
    assert launches("filter") > 0
    return [c.to_numpy() for c in out], rows


def check_filter(ctx, cols, pred, keep, what, out_idx=None):
    """device rows == the oracle's == the input rows NumPy keeps, in input order, bit for bit"""
    got, rows = dev_filter(ctx, cols, pred, out_idx)
    want, wrows, _ = ob.filter(host(cols), pred, out_idx)
    assert rows == wrows == int(keep.sum()), what
    for j, w in enumerate(np_rows(cols, keep, out_idx)):
        assert_bits_equal(got[j], want[j], f"{what} col {j} (oracle)")
        assert_bits_equal(got[j], w, f"{what} col {j} (input rows)")
    return got


def both_terms(cols, op, conn):
    """(expr, keep): `a op -0.0 AND/OR b op' inf`, the non-Kleene connectives (NULL if either side is)"""
    op2 = {"eq": "ne", "ne": "eq", "lt": "ge", "le": "gt", "gt": "le", "ge": "lt"}[op]
    t1, v1 = np_term(cols, 0, op, -0.0)
    t2, v2 = np_term(cols, 1, op2, np.inf)
    e1, e2 = expr_term(0, op, -0.0), expr_term(1, op2, np.inf)
    if conn == "and":
        return e1 & e2, (t1 & t2) & v1 & v2
    return e1 | e2, (t1 | t2) & v1 & v2


@pytest.mark.gpu
@pytest.mark.parametrize("op", sorted(OPS))
def test_filter_generic_program(ctx, op):
    """k_filter's run_program: nullable columns of every type, column-to-column comparisons (Float32
    with negative values and -0.0f against Float64), and the column-to-literal matrix kept out of
    the term form by AND-ing a bare, all-true Boolean column (lower_to_terms takes only compare
    leaves)."""
    for n in SIZES:
        cols = pred_table(n, nulls=True)
        for name, a, b in term_cases(op):
            truth, valid = np_term(cols, a, op, b)
            pred = expr_term(a, op, b)
            if not isinstance(b, int):
                pred = pred & col(4)
            check_filter(ctx, cols, pred, truth & valid, f"{name} n={n}")
        for conn in ("and", "or"):
            pred, keep = both_terms(cols, op, conn)
            check_filter(ctx, cols, pred & col(4), keep, f"{op} {conn} n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("op", sorted(OPS))
def test_filter_terms(ctx, op):
    """eval_terms (compare-to-literal leaves, AND / OR of two) over nullable columns, which keep the
    predicate in k_filter's term form and out of k_filter_fast."""
    for n in SIZES:
        cols = pred_table(n, nulls=True)
        cases = [(name, expr_term(a, op, b), np.logical_and(*np_term(cols, a, op, b)))
                 for name, a, b in term_cases(op) if not isinstance(b, int)]
        cases += [(f"{op} {conn}",) + both_terms(cols, op, conn) for conn in ("and", "or")]
        for name, pred, keep in cases:
            check_filter(ctx, cols, pred, keep, f"{name} n={n}")


@pytest.mark.gpu
@pytest.mark.parametrize("op", sorted(OPS))
def test_filter_fast(ctx, monkeypatch, op):
    """k_filter_fast (non-null 8-byte columns, FastTile-style register tiles): the same rows and
    bits as with QEH_NO_FAST_FILTER=1 (k_filter's term form), the oracle and the input rows."""
    for n in SIZES:
        cols = pred_table(n, nulls=False)[:3]
        cases = [(name, expr_term(a, op, b), np.logical_and(*np_term(cols, a, op, b)))
                 for name, a, b in term_cases(op) if not isinstance(b, int)]
        cases += [(f"{op} {conn}",) + both_terms(cols, op, conn) for conn in ("and", "or")]
        fast = [check_filter(ctx, cols, pred, keep, f"{name} n={n}") for name, pred, keep in cases]
        monkeypatch.setenv("QEH_NO_FAST_FILTER", "1")
        for (name, pred, keep), f in zip(cases, fast):
            slow = check_filter(ctx, cols, pred, keep, f"{name} n={n} (QEH_NO_FAST_FILTER)")
            for j in range(len(cols)):
                assert_bits_equal(slow[j], f[j], f"{name} n={n} col {j}: fast vs term kernel")
        monkeypatch.delenv("QEH_NO_FAST_FILTER")


def f32lit(x):
    return Literal(ScalarValue.Float32(float(x)))


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_projection_arithmetic(ctx, dt):
    """col op col, col op literal and unary minus over the specials.  Unary minus is a sign flip:
    bits.  A binary result that is a NaN (generated, or an operand's carried through) is isnan_only;
    every other result, and validity, by bits."""
    mk = (lambda x: lit(float(x))) if dt == np.float64 else f32lit
    sp = specials_of(dt)
    for n in SIZES:
        cols = [laden(n, dt, 31, nulls=True), laden(n, dt, 32, nulls=True)]
        if n == N_TAIL:  # every special against every special
            a, b = np.meshgrid(sp, sp)
            cols[0][0][:a.size], cols[1][0][:b.size] = a.ravel(), b.ravel()
            cols[0][1][:a.size] = cols[1][1][:b.size] = True
        dev = [ctx.upload(v, m) for v, m in cols]
        exprs = {"neg": UnaryExpr(UnaryOp.Minus, col(0))}
        for name, op in (("add", BinaryOp.Add), ("sub", BinaryOp.Subtract), ("mul", BinaryOp.Multiply),
                         ("div", BinaryOp.Divide)):
            exprs[f"{name} col"] = binop(col(0), op, col(1))
            for x in (sp[1], sp[2], sp[10], sp[6]):  # -0.0, min subnormal, +inf, 1.0
                exprs[f"{name} {x!r}"] = binop(col(0), op, mk(x))
        for name, e in exprs.items():
            out, launches = timed(ctx, lambda: ctx.eval(dev, e))
            assert launches("eval") > 0
            (wv, wm), wdt = ob.eval_expr(host(cols), e, n)
            assert out.dtype == wdt
            assert_bits_equal(out.to_numpy(), (wv, wm), f"{name} n={n}", isnan_only=name != "neg")


# ---- HashAggregate ----------------------------------------------------------------------------
def dev_aggregate(ctx, cols, key_idx, aggs, pred=None):
    dev = [ctx.upload(*c) for c in cols]
    if pred is None:
        fn = lambda: ctx.hash_aggregate([dev[i] for i in key_idx], dev, aggs)
    else:
        fn = lambda: ctx.filter_aggregate(dev, pred, key_idx, aggs)
    (gk, ga, g), launches = timed(ctx, fn)
    assert launches("aggregate_rows") > 0
    return [c.to_numpy() for c in gk], [c.to_numpy() for c in ga], g


def oracle_aggregate(cols, key_idx, aggs, pred=None):
    hc = host(cols)
    if pred is not None:
        fc, _, _ = ob.filter(hc, pred)
        hc = host(fc)
    wk, wa, wg, _ = ob.hash_aggregate([hc[i] for i in key_idx], hc, aggs)
    return wk, wa, wg


# single-key paths: the per-workgroup LDS hash (default), the HBM group table, and k_group_agg_fast
# for non-null 8-byte columns (default; QEH_NO_FAST sends those to the LDS hash kernel)
AGG_TOGGLES = [None, "QEH_NO_LDS_GROUPBY", "QEH_NO_FAST"]


def group_fast_tile(aggs):
    """Rows per k_group_agg_fast tile for non-null inputs, as lds_group_fast sizes it.  State slot 0
    is the group's row count, every aggregate but COUNT takes one more (plan_aggs).  The per-workgroup
    table has 1 + n_slots words per key and up to 2048 keys, halved until it fits 64 KiB; above
    40 KiB the kernel is its 1024-thread variant (8192-row tiles), else 256 threads (2048 rows).
    Only whole tiles go to k_group_agg_fast, the rest to one workgroup of the LDS hash kernel."""
    n_slots = 1 + sum(f != AF.Count for f, _ in aggs)
    lcap = 2048
    while lcap > 256 and (1 + n_slots) * lcap * 8 > 64 * 1024:
        lcap >>= 1
    shm = (1 + n_slots) * lcap * 8
    assert shm <= 64 * 1024
    return (1024 if shm > 40 * 1024 else 256) * 8


def group_fast_sizes(aggs):
    """the working sizes in tiles of k_group_agg_fast: one tile + 1 row, three tiles + 5 rows"""
    t = group_fast_tile(aggs)
    return [t + 1, 3 * t + 5]


# the same five functions in both of k_group_agg_fast's shapes: four value slots make a 40 KiB table
# (256 threads), five a 48 KiB one (1024 threads)
SUM_AGGS_NARROW = [(AF.Sum, 2), (AF.Avg, 2), (AF.Min, 2), (AF.Count, 2)]


def check_aggregate(ctx, monkeypatch, cols, key_idx, aggs, what, pred=None, isnan_only=(), toggles=AGG_TOGGLES):
    wk, wa, wg = oracle_aggregate(cols, key_idx, aggs, pred)
    for env in toggles:
        if env:
            monkeypatch.setenv(env, "1")
        gk, ga, g = dev_aggregate(ctx, cols, key_idx, aggs, pred)
        if env:
            monkeypatch.delenv(env)
        assert g == wg, f"{what} [{env}]: {g} groups, oracle {wg}"
        assert_grouped_bits_equal(gk, ga, wk, wa, isnan_only=isnan_only, what=f"{what} [{env}]")
    return wk, wa, wg


@pytest.mark.gpu
@pytest.mark.parametrize("kdt", [np.float64, np.float32])
@pytest.mark.parametrize("nulls", [True, False])
def test_group_by_float_key_specials(ctx, monkeypatch, kdt, nulls):
    """Float group keys match by bit pattern: -0.0 and +0.0 are two groups with the right sign on
    the output key, every NaN pattern is its own group, the NULL group is separate.  -0.0 is the
    group table's empty marker (INT64_MIN as raw bits).  nulls=False with Float64 keys and values is
    the k_group_agg_fast shape."""
    for n in (N_TAIL, N_MULTI):
        r = rng(n, 41)
        sp = specials_of(kdt)
        key = sp[r.integers(0, 17, n)]
        key[special_positions(n, r, 64)] = sp[1]  # -0.0 in the first lane pair, last row, tile edges
        v, _ = laden(n, np.float64, 42)
        cols = [(key, (r.random(n) > 0.05) if nulls else None), (v, (r.random(n) > 0.1) if nulls else None),
                (exact_summable(r, n), None)]
        aggs = [(AF.Count, 0), (AF.Min, 1), (AF.Max, 1), (AF.Count, 1), (AF.Sum, 2)]
        assert n > group_fast_tile(aggs) == TILE  # nulls=False: whole tiles for k_group_agg_fast
        wk, wa, wg = check_aggregate(ctx, monkeypatch, cols, [0], aggs, f"{kdt.__name__} key n={n}")
        # the oracle's groups are the NumPy groups (so the device's are): 17 patterns (+ NULL)
        gid, rep = np_group_ids(cols[:1])
        assert wg == len(rep) == 17 + (1 if nulls else 0)
        mn, mx, cnt, _, _ = np_min_max_count(cols[:1], cols[1])
        rows = np_min_max_count(cols[:1], cols[0])[2]  # COUNT(key): 0 for the NULL group
        assert_grouped_bits_equal(wk, wa[:4], np_group_keys(cols[:1], rep), [rows, mn, mx, cnt])


@pytest.mark.gpu
@pytest.mark.parametrize("nulls", [True, False])
@pytest.mark.parametrize("groups", [16, 1000])
def test_group_by_min_max_designed(ctx, monkeypatch, groups, nulls):
    """MIN / MAX / COUNT of Float64 and Float32 values over groups whose answers are the signed
    zeros, NaNs of either sign, the order keys INT64_MIN / INT64_MAX, subnormals, infinities and NULL
    (designed_values), through the LDS path, the HBM group table and k_group_agg_fast (nulls=False,
    Float64 values only)."""
    for n in (N_TAIL, N_MULTI):
        cols = agg_table(n, groups, nulls=nulls)
        aggs = MINMAX_AGGS if nulls else [(AF.Min, 1), (AF.Max, 1), (AF.Count, 1), (AF.Sum, 2), (AF.Count, 0)]
        assert nulls or n > group_fast_tile(aggs) == TILE  # whole tiles for k_group_agg_fast
        wk, wa, _ = check_aggregate(ctx, monkeypatch, cols, [0], aggs, f"groups={groups} n={n}")
        mn, mx, cnt, _, rep = np_min_max_count(cols[:1], cols[1])
        assert_grouped_bits_equal(wk, wa[:3], np_group_keys(cols[:1], rep), [mn, mx, cnt])
        if not nulls:  # the same through a predicate term on a special-laden column (filter_aggregate)
            cols.append(laden(n, np.float64, 43))
            check_aggregate(ctx, monkeypatch, cols, [0], aggs, f"groups={groups} n={n} pred",
                            pred=expr_term(5, "gt", -0.0))


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_global_aggregates_specials(ctx, monkeypatch, n):
    """No GROUP BY: MIN / MAX by bits over special-laden Float64 / Float32, exact SUM / AVG.  Global
    aggregates have one path (k_agg_rows with the one group's states in LDS, under the aggregate_rows
    label whose launches dev_aggregate asserts); no toggle selects another."""
    v, w = laden(n, np.float64, 51, nulls=True), laden(n, np.float32, 52, nulls=True)
    x = (exact_summable(rng(n, 53), n), rng(n, 54).random(n) > 0.2)
    aggs = [(AF.Min, 0), (AF.Max, 0), (AF.Count, 0), (AF.Min, 1), (AF.Max, 1), (AF.Sum, 2), (AF.Avg, 2)]
    cols = [v, w, x]
    wk, wa, wg = check_aggregate(ctx, monkeypatch, cols, [], aggs, f"global n={n}", toggles=[None])
    assert wg == 1
    for j, c in ((0, v), (3, w)):  # NumPy: MIN / MAX by totalOrder
        k = np.where(valid_of(c), total_key(c[0]), 0)
        if valid_of(c).any():
            lo = np.flatnonzero(valid_of(c))[np.argmin(k[valid_of(c)])]
            hi = np.flatnonzero(valid_of(c))[np.argmax(k[valid_of(c)])]
            assert_bits_equal(wa[j], (c[0][[lo]], np.ones(1, bool)), f"global MIN col {j}")
            assert_bits_equal(wa[j + 1], (c[0][[hi]], np.ones(1, bool)), f"global MAX col {j}")
    # all-special columns whose extremes are the state's initial values
    for vals in ([MIN_NAN, MAX_NAN, 0.0], [MIN_NAN], [MAX_NAN], [-0.0, 0.0]):
        c = [(np.array(vals, np.float64), None)]
        check_aggregate(ctx, monkeypatch, c, [], [(AF.Min, 0), (AF.Max, 0)], f"global {vals}", toggles=[None])


@pytest.mark.gpu
@pytest.mark.parametrize("nulls", [True, False])
@pytest.mark.parametrize("groups", [7, 1000])
def test_group_by_sum_avg_exact(ctx, monkeypatch, groups, nulls):
    """SUM / AVG of exact_summable values: bit-identical whatever the order of the atomics, AVG one
    correctly rounded division (the oracle's are checked against math.fsum in the CPU half).
    nulls=False is the k_group_agg_fast shape, in both of its variants: SUM_AGGS makes a 64 KiB
    table (1024 threads, 8192-row tiles), SUM_AGGS_NARROW a 40 KiB one (256 threads, 2048-row tiles);
    the sizes are one and three whole tiles of the variant plus a tail, so n_tiles > 0 and the default
    run differs from the QEH_NO_FAST one in the kernel that takes the whole tiles."""
    if nulls:
        for n in (N_TAIL, N_MULTI):
            check_aggregate(ctx, monkeypatch, agg_table(n, groups, nulls=True), [0], SUM_AGGS, f"groups={groups} n={n}")
        return
    assert group_fast_tile(SUM_AGGS) == 4 * TILE and group_fast_tile(SUM_AGGS_NARROW) == TILE
    for aggs in (SUM_AGGS, SUM_AGGS_NARROW):
        for n in group_fast_sizes(aggs):
            assert n // group_fast_tile(aggs) >= 1 and n % group_fast_tile(aggs)
            cols = agg_table(n, groups, nulls=False)
            check_aggregate(ctx, monkeypatch, cols, [0], aggs, f"groups={groups} n={n} {len(aggs)} aggregates")


@pytest.mark.gpu
@pytest.mark.parametrize("nulls", [True, False])
def test_group_by_sum_avg_special_inputs(ctx, monkeypatch, nulls):
    """Groups of only subnormals (exact, not flushed to zero), only -0.0, +inf with finite values
    (+inf), +inf with -inf and a NaN input (both NaN on either side: isnan_only); the remaining
    groups exact_summable.  Everything that is not a NaN by bits.  nulls=False is the
    k_group_agg_fast shape: the five aggregates make its 1024-thread variant (8192-row tiles), the
    four without MAX its 256-thread one (2048-row tiles), each at three whole tiles plus 5 rows, so
    the specials go through the fast kernel's tiles and the default run differs from QEH_NO_FAST's."""
    wide = [(AF.Sum, 1), (AF.Avg, 1), (AF.Count, 1), (AF.Min, 1), (AF.Max, 1)]
    if nulls:
        shapes = [(wide, N_MULTI)]
    else:
        assert group_fast_tile(wide) == 4 * TILE and group_fast_tile(wide[:4]) == TILE
        shapes = [(a, group_fast_sizes(a)[1]) for a in (wide, wide[:4])]
    for aggs, n in shapes:
        r = rng(n, 61)
        gid = r.integers(0, 9, n).astype(np.int64)
        s = exact_summable(r, n)
        s[gid == 0] = r.integers(-1000, 1000, (gid == 0).sum()) * SUB
        s[gid == 1] = -0.0
        s[(gid == 2) & (r.random(n) < 0.2)] = np.inf
        s[gid == 3] = np.where(r.random((gid == 3).sum()) < 0.5, np.inf, -np.inf)
        s[(gid == 4) & (r.random(n) < 0.1)] = POS_NAN
        cols = [(gid, (r.random(n) > 0.05) if nulls else None), (s, (r.random(n) > 0.1) if nulls else None)]
        if not nulls:  # every special group has rows in the whole tiles
            assert set(range(5)) <= set(gid[:n // group_fast_tile(aggs) * group_fast_tile(aggs)].tolist())
        wk, wa, _ = check_aggregate(ctx, monkeypatch, cols, [0], aggs, f"special sums n={n}", isnan_only=(0, 1))
        by = {int(k): i for i, (k, ok) in enumerate(zip(wk[0][0], wk[0][1])) if ok}
        sums = wa[0][0]
        sub_sum = math.fsum(s[(gid == 0) & valid_of(cols[0]) & valid_of(cols[1])].tolist())
        assert sums[by[0]] == sub_sum != 0.0 and abs(sub_sum) < 2.3e-308  # a subnormal sum, not flushed
        assert sums[by[2]] == np.inf and np.isnan(sums[by[3]]) and np.isnan(sums[by[4]])

@pytest.mark.gpu
@pytest.mark.parametrize("order", ["float_int", "int_float"])
@pytest.mark.parametrize("kdt", [np.float64, np.float32])
def test_group_by_multi_key_specials(ctx, monkeypatch, order, kdt):
    """(float key, int key) and (int key, float key) through the multi-key group table."""
    for n in (N_TAIL, N_MULTI):
        r = rng(n, 71)
        fk = (specials_of(kdt)[r.integers(0, 17, n)], r.random(n) > 0.05)
        ik = (r.integers(0, 3, n).astype(np.int64), r.random(n) > 0.05)
        v = laden(n, np.float64, 72, nulls=True)
        cols = [fk, ik, v, (exact_summable(r, n), None)] if order == "float_int" else [ik, fk, v, (exact_summable(r, n), None)]
        aggs = [(AF.Count, 0), (AF.Min, 2), (AF.Max, 2), (AF.Sum, 3), (AF.Avg, 3)]
        wk, wa, wg = check_aggregate(ctx, monkeypatch, cols, [0, 1], aggs, f"{order} n={n}", toggles=[None])
        gid, rep = np_group_ids(cols[:2])
        mn, mx, _, _, _ = np_min_max_count(cols[:2], v)
        rows = np_min_max_count(cols[:2], cols[0])[2]  # COUNT(first key): 0 where it is NULL
        assert wg == len(rep)
        assert_grouped_bits_equal(wk, wa[:3], np_group_keys(cols[:2], rep), [rows, mn, mx])


@pytest.mark.gpu
@pytest.mark.parametrize("keys", [[0], [0, 4]])
def test_more_than_eight_aggregates_float_min_max(ctx, monkeypatch, keys):
    """The >8-aggregate chunking with float MIN / MAX on both sides of the chunk boundary (aggregates
    6, 7 and 8, 9)."""
    cols = agg_table(N_MULTI, 16)
    aggs = [(AF.Sum, 2), (AF.Count, 1), (AF.Avg, 2), (AF.Count, 0), (AF.Min, 3), (AF.Max, 3), (AF.Min, 1), (AF.Max, 1),
            (AF.Max, 1), (AF.Min, 1), (AF.Max, 3), (AF.Min, 3)]
    check_aggregate(ctx, monkeypatch, cols, keys, aggs, f"12 aggregates keys={keys}", toggles=[None])


# ---- fused join-aggregate ----------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("litv,op", [(-0.0, "gt"), (-0.0, "le"), (np.inf, "lt"), (np.inf, "ge")])
def test_join_filter_aggregate_specials(ctx, monkeypatch, litv, op):
    """Probe of 3 tiles + 5 rows against a ~1000-row build: the predicate term's column carries the
    specials, SUM / AVG over exact_summable values, MIN / MAX over special-laden ones.  At this size
    the defaults, QEH_NO_FUSED and QEH_NO_SLICES all end in the general path (join table + probe
    kernel; by default only after the fused pipeline's device plan turned the 2 KB table down), so
    QEH_SLICE_MIN_BYTES=0 forces the fused slice pipeline: two aggregate columns make its tiles 4096
    rows, the probe is one whole tile and a partial one.  Each run asserts its path's labels; all
    are bit-equal to the oracle."""
    n, nd = N_MULTI, 1000
    r = rng(n, 81)
    probe = [laden(n, np.float64, 82), (r.integers(-20, nd + 20, n).astype(np.int64), None),
             (exact_summable(r, n), None), laden(n, np.float64, 83)]
    dk = r.permutation(nd).astype(np.int64)
    dg = r.integers(0, 16, nd).astype(np.int64)
    pred = expr_term(0, op, litv)
    aggs = [(AF.Sum, 2), (AF.Avg, 2), (AF.Min, 3), (AF.Max, 3), (AF.Count, 2)]
    wk, wa, wg = ob.join_filter_aggregate(host(probe), 1, pred, ob.HostCol(dk), [ob.HostCol(dg)], aggs)
    # NumPy: the rows the predicate keeps and the join matches, grouped by the build side's group key
    keep = np.logical_and(*np_term(probe, 0, op, litv)) & (probe[1][0] >= 0) & (probe[1][0] < nd)
    g_of_key = np.empty(nd, np.int64)
    g_of_key[dk] = dg
    gkey = [(g_of_key[probe[1][0][keep]], None)]
    mn, mx, cnt, _, rep = np_min_max_count(gkey, (probe[3][0][keep], None))
    assert_grouped_bits_equal(wk, [wa[2], wa[3], wa[4]], np_group_keys(gkey, rep), [mn, mx, cnt], what="oracle vs numpy")
    for env in (None, "QEH_NO_FUSED", "QEH_NO_SLICES", "QEH_SLICE_MIN_BYTES"):
        if env:
            monkeypatch.setenv(env, "0" if env == "QEH_SLICE_MIN_BYTES" else "1")
        dev = [ctx.upload(*c) for c in probe]
        (gk, ga, g), launches = timed(ctx, lambda: ctx.join_filter_aggregate(dev, 1, pred, ctx.upload(dk), [ctx.upload(dg)], aggs))
        ran = {k: launches(k) for k in ("join_filter_aggregate", "slice_probe", "fused_build", "fused_build_declined")}
        if env:
            monkeypatch.delenv(env)
        if env == "QEH_SLICE_MIN_BYTES":  # the fused pipeline: build rows by slice, phase A, phase B
            assert ran["fused_build"] > 0 and ran["slice_probe"] > 0 and ran["join_filter_aggregate"] == 0, ran
        else:  # the general path: join table, then the probe kernel under the operator's own label
            assert ran["join_filter_aggregate"] > 0 and ran["slice_probe"] == ran["fused_build"] == 0, (env, ran)
            # by default the fused pipeline is tried and its device plan declines (a 2 KB table)
            assert (ran["fused_build_declined"] > 0) == (env is None), (env, ran)
        assert g == wg
        assert_grouped_bits_equal([c.to_numpy() for c in gk], [c.to_numpy() for c in ga], wk, wa, what=f"[{env}]")


# ---- Sort --------------------------------------------------------------------------------------
def dev_sort(ctx, keys, asc, nf=None):
    dev = [ctx.upload(*k) for k in keys]
    fn = (lambda: ctx.sort_indices(dev, asc)) if nf is None else (lambda: ctx.sort_indices_nulls(dev, asc, nf))
    out, launches = timed(ctx, fn)
    if len(keys[0][0]) > 1:
        assert launches("radix_pass") > 0 and launches("sort_encode") > 0
    return out.to_numpy()[0]


# 8192 rows is the radix scatter's tile: from there a pass also writes the next pass's digits
SORT_SIZES = [7, N_TAIL, N_MULTI, 8192 + 3]


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n", SORT_SIZES)
def test_sort_specials_single_key(ctx, dt, n):
    """The LSD radix passes over a special-laden key.  With NULLs the Float64 key holds both
    0x7FFF...F and 0xFFFF...F, so its order keys span all of Int64 and no code is left for NULL (the
    float twin of full_range_nulls_last): the null-flag pass.  Permutation == oracle == NumPy."""
    for nulls in (True, False):
        keys = sort_keys(n, dt, nulls)[:1]
        if n >= N_TAIL and dt == np.float64:
            assert {0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF} <= set(keys[0][0][valid_of(keys[0])].view(np.uint64).tolist())
        for asc, nf in SORT_MODES:
            got = dev_sort(ctx, keys, [asc], [nf])
            assert np.array_equal(got, ob.sort_indices_nulls(host(keys), [asc], [nf])), (nulls, asc, nf)
            assert np.array_equal(got, np_sort_perm(keys, [asc], [nf])), (nulls, asc, nf)
        for asc in (True, False):
            got = dev_sort(ctx, keys, [asc])
            assert np.array_equal(got, ob.sort_indices(host(keys), [asc])), (nulls, asc)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n", SORT_SIZES)
def test_sort_specials_with_secondary_key(ctx, monkeypatch, dt, n):
    """(special-laden float, Int64) and (Int64, special-laden float).  The float key's order keys span
    all 64 bits.  Non-null (Int64, float): the first key needs 3 bits, so sort_perm_pair takes its
    truncated pair encoding (the Int64 key over the float key's top bits) and k_fix_pair_runs orders
    the runs of equal codes by the dropped low bits, falling back to one sort per column only if a
    run is longer than 64 rows.  Non-null (float, Int64), and every order with NULLs, is declined by
    the pair sort and takes one sort per column.  The pair branches share the sort_encode label with
    the per-column encode, so the path is pinned by QEH_NO_PAIR_SORT=1 (always one sort per column),
    which must give the same permutation."""
    for nulls in (True, False):
        fk, ik = sort_keys(n, dt, nulls)
        for keys in ([fk, ik], [ik, fk]):
            for asc, nf in SORT_MODES:
                want = ob.sort_indices_nulls(host(keys), [asc, not asc], [nf, not nf])
                assert np.array_equal(want, np_sort_perm(keys, [asc, not asc], [nf, not nf]))
                got = dev_sort(ctx, keys, [asc, not asc], [nf, not nf])
                assert np.array_equal(got, want), (nulls, asc, nf)
                monkeypatch.setenv("QEH_NO_PAIR_SORT", "1")
                got = dev_sort(ctx, keys, [asc, not asc], [nf, not nf])
                monkeypatch.delenv("QEH_NO_PAIR_SORT")
                assert np.array_equal(got, want), (nulls, asc, nf, "QEH_NO_PAIR_SORT")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("n", SORT_SIZES)
def test_sort_pair_path_signed_zeros_and_subnormals(ctx, monkeypatch, dt, n):
    """The two-key pair encoding needs both keys' order-key spans to fit 64 bits together: non-null
    keys, the float one drawn from {+-0.0, +-1, +-2, +-3 subnormal steps} (order keys -4 .. 3, where
    -0.0 = -1 sits right below +0.0 = 0).  Same permutation with QEH_NO_PAIR_SORT=1 (one sort per
    column), the oracle's and NumPy's."""
    r = rng(n, 91)
    tiny = np.array([0, 1, 2, 3], np.uint64 if dt == np.float64 else np.uint32)
    sign = np.array(1, tiny.dtype) << np.array(63 if dt == np.float64 else 31, tiny.dtype)
    vals = np.concatenate([tiny, tiny | sign]).view(dt)
    fk = (vals[r.integers(0, 8, n)], None)
    ik = (r.integers(-50, 50, n).astype(np.int64), None)
    for keys in ([fk, ik], [ik, fk]):
        for asc in ([True, True], [False, True], [True, False]):
            want = ob.sort_indices(host(keys), asc)
            assert np.array_equal(want, np_sort_perm(keys, asc, [True, True]))
            got = dev_sort(ctx, keys, asc)
            assert np.array_equal(got, want), asc
            monkeypatch.setenv("QEH_NO_PAIR_SORT", "1")
            got = dev_sort(ctx, keys, asc)
            monkeypatch.delenv("QEH_NO_PAIR_SORT")
            assert np.array_equal(got, want), (asc, "QEH_NO_PAIR_SORT")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_sort_limit_specials(ctx, monkeypatch, dt):
    """ORDER BY ... LIMIT over a special-laden key: the first rows of the full sort from the top-k
    radix select (QEH_TOPK_MIN_ROWS=0 lets it run below 2^22 rows; it takes limits under n / 16) and
    the same rows with QEH_NO_TOPK=1 (full sort, then cut).  A nullable Float64 key holding both
    all-ones NaNs spans 2^64 order keys plus NULL, which the select declines: the full sort answers."""
    monkeypatch.setenv("QEH_TOPK_MIN_ROWS", "0")
    for n in (N_TAIL, N_MULTI):
        for nulls in (False, True):
            keys = sort_keys(n, dt, nulls=nulls)[:1]
            select_takes_it = not (nulls and dt == np.float64)
            for asc in (True, False):
                want = ob.sort_indices(host(keys), [asc])
                for limit in (1, 40, n // 16 - 1, n - 1):
                    dev = [ctx.upload(*k) for k in keys]
                    out, launches = timed(ctx, lambda: ctx.sort_indices_limit(dev, [asc], limit))
                    assert (launches("topk_select") > 0) == (select_takes_it and limit < n // 16), (n, nulls, asc, limit)
                    monkeypatch.setenv("QEH_NO_TOPK", "1")
                    full, launches = timed(ctx, lambda: ctx.sort_indices_limit(dev, [asc], limit))
                    monkeypatch.delenv("QEH_NO_TOPK")
                    assert launches("topk_select") == 0
                    assert np.array_equal(out.to_numpy()[0], want[:limit]), (n, nulls, asc, limit)
                    assert np.array_equal(full.to_numpy()[0], want[:limit]), (n, nulls, asc, limit, "QEH_NO_TOPK")


# ---- Window ------------------------------------------------------------------------------------
def np_ranks(part, key, asc):
    """(ROW_NUMBER, RANK, DENSE_RANK) by totalOrder peers: equal bits are peers, nothing else is"""
    n = len(part)
    k = total_key(key)
    order = np.lexsort((np.arange(n), k if asc else ~k, part))
    p, q = part[order], k[order]
    new_part = np.r_[True, p[1:] != p[:-1]]
    new_peer = new_part | np.r_[True, q[1:] != q[:-1]]
    idx = np.arange(n)
    start = np.maximum.accumulate(np.where(new_part, idx, 0))
    peer = np.maximum.accumulate(np.where(new_peer, idx, 0))
    dense = np.cumsum(new_peer)
    dense = dense - dense[start] + 1
    out = np.empty((3, n), np.int64)
    out[:, order] = [idx - start + 1, peer - start + 1, dense]
    return out


WINDOW_PATHS = {
    # name: (environment, the label whose launches prove the path, labels that must not have run)
    "lsd": ({"QEH_NO_WINDOW_MSD": "1"}, "radix_pass", ("window_sort", "w3_place")),
    "msd": ({"QEH_WINDOW_MSD": "1"}, "window_sort", ("w3_place",)),
    "w3": ({"QEH_WINDOW_MSD": "1", "QEH_WINDOW_W3": "1"}, "w3_place", ("window_sort",)),
}


def window_data(n, dt, parts):
    r = rng(n, parts, 101)
    part = r.integers(0, parts, n).astype(np.int64) + 1000
    return part, laden(n, dt, 102)[0]


@pytest.mark.gpu
@pytest.mark.parametrize("path", sorted(WINDOW_PATHS))
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_window_ranking_specials(ctx, monkeypatch, path, dt):
    """ROW_NUMBER / RANK / DENSE_RANK ordered by a special-laden float key on each window path: the
    per-column LSD sort, the partitioning path (window_sort) and the three-level pipeline (w3_place;
    it declines DENSE_RANK, which then takes the partitioning path).  -0.0 and +0.0 are different
    peers, equal-bits NaNs are peers, different payloads are not."""
    env, label, absent = WINDOW_PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for n, parts in ((N_TAIL, 32), (N_MULTI, 96)):  # ~64-row partitions: a few rows per special in each
        part, key = window_data(n, dt, parts)
        for asc in (True, False):
            want = np_ranks(part, key, asc)
            for i, func in enumerate((W.RowNumber, W.Rank, W.DenseRank)):
                dp, dk = ctx.upload(part), ctx.upload(key)
                if func == W.RowNumber:
                    out, launches = timed(ctx, lambda: ctx.row_number([dp], [dk], [asc]))
                    ref = ob.row_number([ob.HostCol(part)], [ob.HostCol(key)], [asc])
                else:
                    out, launches = timed(ctx, lambda: ctx.window(func, [dp], [dk], [asc]))
                    ref, _ = ob.window(func, [ob.HostCol(part)], [ob.HostCol(key)], [asc])
                if path == "w3" and func == W.DenseRank:
                    assert launches("w3_place") == 0 and launches("window_sort") > 0
                else:
                    assert launches(label) > 0, (path, func, n)
                    assert all(launches(a) == 0 for a in absent), (path, func, n)
                got = out.to_numpy()[0]
                assert np.array_equal(ref, want[i]), (func, n, asc, "oracle vs numpy")
                assert np.array_equal(got, ref), (path, func, n, asc)


VALUE_FUNCS = [(W.Lag, 1), (W.Lead, 2), (W.FirstValue, 0), (W.LastValue, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_window_value_functions_special_argument(ctx, monkeypatch, dt):
    """LAG / LEAD / FIRST_VALUE / LAST_VALUE copy the argument's bits (NaN payloads, -0.0): a nullable
    special-laden argument ordered by an Int64 key, with and without a default."""
    monkeypatch.setenv("QEH_NO_WINDOW_MSD", "1")
    for n in (N_TAIL, N_MULTI):
        part, _ = window_data(n, dt, 32)
        okey = rng(n, 111).integers(-20, 20, n).astype(np.int64)
        arg = laden(n, dt, 112, nulls=True)
        for func, param in VALUE_FUNCS:
            for default in (None, specials_of(dt)[1]):  # -0.0 as the default
                if default is not None and func not in (W.Lag, W.Lead):
                    continue
                out, launches = timed(ctx, lambda: ctx.window(func, [ctx.upload(part)], [ctx.upload(okey)], [True],
                                                              arg=ctx.upload(*arg), param=param, default=default))
                assert launches("window") > 0 and launches("window_sort") == 0
                want = ob.window(func, [ob.HostCol(part)], [ob.HostCol(okey)], [True], arg=ob.HostCol(*arg), param=param,
                                 default=default)
                assert_bits_equal(out.to_numpy(), want, f"func {func} n={n} default={default}")


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["lsd", "msd"])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_window_value_functions_of_special_order_key(ctx, monkeypatch, path, dt):
    """Value functions whose argument is the special-laden ORDER BY column itself: the partitioning
    path decodes the value back from its order key, which must give back the input bits."""
    env, label, absent = WINDOW_PATHS[path]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    for n, parts in ((N_TAIL, 32), (N_MULTI, 96)):
        part, key = window_data(n, dt, parts)
        for asc in (True, False):
            for func, param in VALUE_FUNCS:
                dk = ctx.upload(key)
                out, launches = timed(ctx, lambda: ctx.window(func, [ctx.upload(part)], [dk], [asc], arg=dk, param=param))
                assert launches(label) > 0 and all(launches(a) == 0 for a in absent), (path, func, n)
                want = ob.window(func, [ob.HostCol(part)], [ob.HostCol(key)], [asc], arg=ob.HostCol(key), param=param)
                assert_bits_equal(out.to_numpy(), want, f"{path} func {func} n={n} asc={asc}")


# ---- Merge and range partition -------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_merge_sorted_special_float_keys(ctx, dt):
    """Merge::sorted of 3 partitions on a special-laden nullable float key with an Int64 payload: key
    bits, validity and payload equal the stable sort of the concatenation (oracle and NumPy)."""
    sizes = [N_TAIL, 7, N_MULTI]
    n = sum(sizes)
    key = laden(n, dt, 121, nulls=True)
    pay = np.arange(n, dtype=np.int64) * 3 - n
    cuts = np.r_[0, np.cumsum(sizes)]
    for asc, nf in SORT_MODES:
        parts = [[ctx.upload(key[0][a:b], key[1][a:b]), ctx.upload(pay[a:b])] for a, b in zip(cuts[:-1], cuts[1:])]
        (cols, rows), launches = timed(ctx, lambda: ctx.merge_sorted(parts, [0], [asc], [nf]))
        assert rows == n and launches("radix_pass") > 0
        perm = ob.sort_indices_nulls(host([key]), [asc], [nf])
        assert np.array_equal(perm, np_sort_perm([key], [asc], [nf]))
        assert_bits_equal(cols[0].to_numpy(), (key[0][perm], key[1][perm]), f"key asc={asc} nf={nf}")
        assert_bits_equal(cols[1].to_numpy(), (pay[perm], None), f"payload asc={asc} nf={nf}")


@pytest.mark.gpu
def test_merge_sorted_msd_special_float_payload(ctx, monkeypatch):
    """A float key cannot reach the payload sort or its MSD passes: they take Int32 / Int64 keys only,
    and a merge on a float key goes through the permutation sort (the test above).  Here the float is
    a payload, copied through the passes and never compared: it must arrive bit for bit.  2^20 rows
    and a 30-bit key range are the smallest shape that takes the MSD passes (n >= 2^20, >= 24 code
    bits).  The MSD passes record two radix_pass stages and, had a sub-bucket been too large
    (kMsdRedo), the LSD passes would follow under the same label, so exactly two shows that the MSD
    passes gave the answer; QEH_NO_MSD_SORT=1 records one stage per 8-bit LSD pass (four for these
    codes) and QEH_NO_PAYLOAD_SORT=1 sorts a permutation and gathers."""
    n = 1 << 20
    r = rng(n, 131)
    k = r.integers(0, 2 ** 30, n, dtype=np.int64)
    kv = r.random(n) > 0.05
    pay = laden(n, np.float64, 132)[0]
    cuts = [0, n // 3, n // 3 + 7, n]
    parts = [[ctx.upload(k[a:b], kv[a:b]), ctx.upload(pay[a:b])] for a, b in zip(cuts[:-1], cuts[1:])]
    perm = ob.sort_indices_nulls([ob.HostCol(k, kv)], [False], [False])
    for env in (None, "QEH_NO_MSD_SORT", "QEH_NO_PAYLOAD_SORT"):
        if env:
            monkeypatch.setenv(env, "1")
        (cols, rows), launches = timed(ctx, lambda: ctx.merge_sorted(parts, [0], [False], [False]))
        if env:
            monkeypatch.delenv(env)
        passes = launches("radix_pass")
        assert rows == n
        if env is None:
            assert passes == 2, passes  # the MSD passes, and no LSD passes after them
        elif env == "QEH_NO_MSD_SORT":
            assert passes == 4, passes  # codes of 25..32 bits (a range under 2^30, + the NULL code): four 8-bit passes
        assert_bits_equal(cols[0].to_numpy(), (k[perm], kv[perm]), f"key [{env}]")
        assert_bits_equal(cols[1].to_numpy(), (pay[perm], None), f"payload [{env}]")


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("asc", [True, False])
def test_range_partition_special_splitters(ctx, dt, asc):
    """Splitters [-inf, -0.0, 0.0, a positive NaN] over a column holding every special (and NULLs,
    which go to partition 0): membership by totalOrder, input order inside a partition."""
    split = np.sort(total_key(np.array([-np.inf, -0.0, 0.0, POS_NAN])))
    for n in (N_TAIL, N_MULTI):
        v, m = laden(n, dt, 141, nulls=True)
        assert set(bits_of(specials_of(dt)).tolist()) <= set(bits_of(v[m]).tolist())
        (counts, perm), launches = timed(ctx, lambda: ctx.range_partition(ctx.upload(v, m), split, asc))
        assert launches("range_partition") > 0
        p = perm.to_numpy()[0]
        k = total_key(v)
        part = (split[None, :] < k[:, None]).sum(1) if asc else (split[None, :] > k[:, None]).sum(1)
        part = np.where(m, part, 0)
        assert np.array_equal(counts, np.bincount(part, minlength=5)), (n, counts)
        assert np.array_equal(p, np.lexsort((np.arange(n), part)).astype(np.uint32)), n
