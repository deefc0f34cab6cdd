"""IN / EXISTS / scalar subquery expressions: qeh_in_set (k_semi.hip) and the plan executor's
rewrite_subqueries.

qeh_in_set is a semi join (anti join when negated) that yields one nullable bit per probe row.  Its
set is a bitmap over the key range or a key-only hash set; QEH_IN_SET forces one.  Expected values
never come from the code under test: `rule()` below is SQL's three-valued IN written out in Python
over sets of key bits (np.isin's answer plus the NULL rule), and the plan-level answers on
tests/golden/employees.csv x departments.csv are derived by hand:

    employees   id name    age salary dept_id        departments  dept_id
                1  Alice   25  75000  101                         101
                2  Bob     30  85000  102                         102
                3  Charlie 35  95000  101                         103
                4  Diana   28  80000  103                         104
                5  Eve     32  90000  102
                6  Frank   29  78000  NULL           AVG(salary) = 503000 / 6 = 83833.33
"""
import os
import re
import zlib

import numpy as np
import pyarrow.csv as pacsv
import pytest

import qe_hip
from qe_hip import (AggregateExpr, AggregateFunction as AF, BinaryOp, Exists, Filter, HashAggregate, HashJoin,
                    InSubquery, JoinType, Limit, MemoryDataSource, Projection, QueryExecutor, ScalarSubquery, Scan,
                    UnaryExpr, UnaryOp, abi, binop, col, lit)
from qe_hip.plan import PLAN_PROJECTION, _Flattener

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
M64 = (1 << 64) - 1


# ---- the rule -------------------------------------------------------------------------------------

def key_bits(a):
    """A column's values as the keys IN compares: integers by value, floats by their bit pattern."""
    a = np.asarray(a)
    if a.dtype == np.float64:
        return [int(x) for x in a.view(np.int64)]
    if a.dtype == np.float32:
        return [int(x) for x in a.view(np.int32)]
    if a.dtype == object:
        return [x if isinstance(x, bytes) or x is None else x.encode() for x in a]
    return [int(x) for x in a]


def rule(pk, pm, sk, sm, negated):
    """(values, valid) of `p [NOT] IN (s)` by SQL three-valued logic; pk / sk: keys, pm / sm: validity."""
    n = len(pk)
    if len(sk) == 0:  # no rows at all: decided, even for a NULL probe
        return np.full(n, bool(negated)), np.ones(n, bool)
    have = {k for k, m in zip(sk, sm) if m}
    has_null = not all(sm)
    vals, valid = np.zeros(n, bool), np.zeros(n, bool)
    for i, (k, m) in enumerate(zip(pk, pm)):
        if not m:
            continue
        if k in have:
            vals[i], valid[i] = not negated, True
        elif not has_null:
            vals[i], valid[i] = bool(negated), True
    return vals, valid


def run_in_set(ctx, pc, sc, negated):
    out = ctx.in_set(pc, sc, negated)
    assert out.dtype == abi.DT_BOOL and len(out) == len(pc)
    vals, valid = out.to_numpy()
    if valid is None:
        valid = np.ones(len(vals), bool)
    return vals, valid


def check(ctx, p, pm, s, sm, negated, poff=0, soff=0):
    pm = np.ones(len(p), bool) if pm is None else np.asarray(pm, bool)
    sm = np.ones(len(s), bool) if sm is None else np.asarray(sm, bool)
    pc = ctx.upload(p, None if pm.all() and poff == 0 else pm, offset=poff)
    sc = ctx.upload(s, None if sm.all() and soff == 0 else sm, offset=soff)
    vals, valid = run_in_set(ctx, pc, sc, negated)
    want_vals, want_valid = rule(key_bits(p), pm, key_bits(s), sm, negated)
    assert np.array_equal(valid, want_valid), (len(p), len(s), negated)
    assert np.array_equal(vals[valid], want_vals[want_valid]), (len(p), len(s), negated)


def hash64(k):  # device_common.h hash64 (murmur3 fmix64): the hash set's home slot is hash64(key) & (capacity - 1)
    k &= M64
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M64
    k ^= k >> 33
    return k


def form_used(ctx, fn):
    """Run fn() with kernel timing on; which probe kernel ran."""
    ctx.timing(True)
    ctx.timing_reset()
    try:
        fn()
        return {f: ctx.kernel_time("semi_probe_" + f)[1] for f in ("bitmap", "hash")}
    finally:
        ctx.timing(False)


# ---- CPU: the boundary ------------------------------------------------------------------------------

def test_in_set_is_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "qeh.h")).read()
    assert "#define QEH_ABI_VERSION 1" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"^\s*int\s+qeh_in_set\s*\(([^)]*)\)\s*;", code, flags=re.M)
    assert m and m.group(1).count("qeh_column") == 3 and "int negated" in m.group(1)
    for name, v in [("QEH_EX_SCALAR_SUBQUERY", 5), ("QEH_EX_IN_SUBQUERY", 6), ("QEH_EX_EXISTS", 7)]:
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, v), code), name
    assert (abi.EX_SCALAR_SUBQUERY, abi.EX_IN_SUBQUERY, abi.EX_EXISTS) == (5, 6, 7)
    assert len(abi.SIGNATURES["qeh_in_set"][1]) == 5
    assert hasattr(qe_hip.load(), "qeh_in_set")
    assert hasattr(qe_hip.Context, "in_set")


class _NoSource(qe_hip.DataSource):
    pass


def test_flattener_emits_the_subplan_and_points_the_node_at_its_root():
    emp, dep = _NoSource(), _NoSource()
    sub = Projection(Filter(Scan(dep), binop(col(0), BinaryOp.Greater, lit(101))), [col(0)], ["dept_id"])
    plan = Filter(Scan(emp), InSubquery(col(4), sub, negated=True) & Exists(Scan(dep)))
    fl = _Flattener()
    root = fl.add(plan)
    # the outer scan, IN's subplan (scan, filter, projection), EXISTS' scan, the outer filter
    assert len(fl.nodes) == 6 and root == 5
    assert fl.sources == [emp, dep, dep]
    pred = fl.nodes[root].predicate
    nodes = [pred.nodes[i] for i in range(pred.n_nodes)]
    assert [n.kind for n in nodes] == [abi.EX_COLUMN, abi.EX_IN_SUBQUERY, abi.EX_EXISTS, abi.EX_BINARY]
    assert nodes[1].op == 1 and nodes[2].op == 0
    assert fl.nodes[nodes[1].index].kind == PLAN_PROJECTION  # the subplan's root
    inner = fl.nodes[fl.nodes[nodes[1].index].input]
    assert inner.has_predicate == 1 and fl.nodes[inner.input].source == 1
    assert fl.nodes[nodes[2].index].source == 2
    # a scalar subquery is a leaf with the same fields
    fl2 = _Flattener()
    r2 = fl2.add(Filter(Scan(emp), binop(col(3), BinaryOp.Greater, ScalarSubquery(Scan(dep)))))
    p2 = fl2.nodes[r2].predicate
    assert [p2.nodes[i].kind for i in range(3)] == [abi.EX_COLUMN, abi.EX_SCALAR_SUBQUERY, abi.EX_BINARY]
    assert fl2.nodes[p2.nodes[1].index].source == 1


def test_to_c_is_unchanged_for_plain_expressions_and_refuses_subqueries_without_a_plan():
    e, keep = binop(binop(col(2), BinaryOp.Add, lit(1)), BinaryOp.Less, lit(2.5)).to_c()
    assert e.n_nodes == 5
    assert [e.nodes[i].kind for i in range(5)] == [abi.EX_COLUMN, abi.EX_LITERAL, abi.EX_BINARY, abi.EX_LITERAL,
                                                   abi.EX_BINARY]
    assert e.nodes[0].index == 2 and e.nodes[1].lit_i64 == 1 and e.nodes[3].lit_f64 == 2.5
    assert len(keep) == 2
    with pytest.raises(ValueError):
        InSubquery(col(0), Scan(_NoSource())).to_c()


@pytest.mark.parametrize("kind", [5, 6, 7])
def test_typing_an_expression_with_a_subquery_outside_a_plan_is_refused(kind):
    lib = qe_hip.load()
    nodes = [abi.QehExprNode(kind=abi.EX_COLUMN, index=0), abi.QehExprNode(kind=kind, index=0)]
    arr = (abi.QehExprNode * 2)(*nodes)
    e = abi.QehExpr(arr, 2)
    dts = (abi.C.c_int32 * 1)(abi.DT_INT64)
    out = abi.C.c_int32()
    assert lib.qeh_expr_type(dts, 1, abi.C.byref(e), abi.C.byref(out)) == abi.QEH_E_UNSUPPORTED
    assert b"subquery expression outside a plan" in lib.qeh_last_error()


# ---- GPU: qeh_in_set against the rule --------------------------------------------------------------

PROBE_SIZES = [0, 1, 63, 64, 65, 4097]  # word boundaries, a partial last word, several tiles and waves
SET_SIZES = [0, 1, 1000]                # none, one, many with duplicates (1000 draws of 100 values)


@pytest.mark.gpu
@pytest.mark.parametrize("offsets", [(0, 0), (3, 5)], ids=["off0", "off3_5"])
@pytest.mark.parametrize("nulls", ["none", "probe", "set", "both"])
@pytest.mark.parametrize("negated", [False, True], ids=["in", "not_in"])
@pytest.mark.parametrize("form", ["bitmap", "hash"])
def test_in_set_matches_the_rule(ctx, monkeypatch, form, negated, nulls, offsets):
    monkeypatch.setenv("QEH_IN_SET", form)
    rng = np.random.default_rng(zlib.crc32(repr((form, negated, nulls, offsets)).encode()))
    for n in PROBE_SIZES:
        for m in SET_SIZES:
            p = rng.integers(-50, 150, n).astype(np.int64)
            s = rng.integers(0, 100, m).astype(np.int64)
            pm = rng.random(n) > 0.3 if nulls in ("probe", "both") else None
            sm = rng.random(m) > 0.3 if nulls in ("set", "both") else None
            if sm is not None and m == 1:
                sm[:] = False  # a set of one NULL: nothing is found, nothing is decided
            check(ctx, p, pm, s, sm, negated, *offsets)


@pytest.mark.gpu
@pytest.mark.parametrize("negated", [False, True])
def test_empty_set_decides_even_null_probes(ctx, negated):
    p = np.arange(130, dtype=np.int64)
    pm = np.arange(130) % 3 != 0
    vals, valid = run_in_set(ctx, ctx.upload(p, pm), ctx.upload(np.zeros(0, np.int64)), negated)
    assert valid.all() and (vals == negated).all()


@pytest.mark.gpu
def test_bitmap_many_lanes_one_word_and_range_edges(ctx, monkeypatch):
    # every key of 0..63 and of 64..95 in one call: 32 lanes of a wave hit each 32-bit word
    s = np.random.default_rng(1).permutation(np.arange(0, 96)).astype(np.int64)
    p = np.concatenate([np.array([-1, 0, 95, 96], np.int64), np.arange(-100, 200, dtype=np.int64)])  # min-1, min, max, max+1
    used = form_used(ctx, lambda: check(ctx, p, None, s, None, False))
    assert used == {"bitmap": 1, "hash": 0}  # a dense range picks the bitmap by itself
    monkeypatch.setenv("QEH_IN_SET", "bitmap")
    for negated in (False, True):
        check(ctx, p, None, s, None, negated)
        check(ctx, p, p % 7 != 0, s, s % 5 != 0, negated, 1, 7)
    # only the two ends of the range set
    check(ctx, p, None, np.array([0, 95], np.int64), None, False)
    monkeypatch.setenv("QEH_IN_SET", "hash")
    assert form_used(ctx, lambda: check(ctx, p, None, s, None, False)) == {"bitmap": 0, "hash": 1}


@pytest.mark.gpu
def test_hash_chain_of_64_keys_with_one_home_slot(ctx, monkeypatch):
    monkeypatch.setenv("QEH_IN_SET", "hash")
    cap = 128  # 64 set rows -> capacity 2 * 64
    same = [k for k in range(1, 40000) if hash64(k) & (cap - 1) == 5]
    assert len(same) >= 128
    s = np.array(same[:64], np.int64)
    p = np.array(same[:128] + list(range(-20, 20)), np.int64)  # present, absent on the same chain, others
    for negated in (False, True):
        check(ctx, p, None, s, None, negated)


@pytest.mark.gpu
def test_hash_reserved_empty_value_is_a_key(ctx, monkeypatch):
    monkeypatch.setenv("QEH_IN_SET", "hash")
    p = np.array([-1, 0, 1, -2, -1], np.int64)  # -1 has the bits of an empty slot
    check(ctx, p, None, np.array([5, -1, 7, -1], np.int64), None, False)
    check(ctx, p, None, np.array([5, 6, 7], np.int64), None, False)
    check(ctx, p, None, np.array([5, -1, 7], np.int64), [True, False, True], True)  # -1 only as a NULL's filler
    f = np.array([np.float32(1.0)] * 3, np.float32).view(np.int32)
    f[1] = -1  # a NaN whose 32 bits sign-extend to the empty value
    check(ctx, f.view(np.float32), None, f.view(np.float32)[1:], None, False)


@pytest.mark.gpu
def test_int64_extremes_do_not_pick_the_bitmap(ctx):
    lo, hi = np.iinfo(np.int64).min, np.iinfo(np.int64).max
    s = np.array([lo, hi, 0], np.int64)
    p = np.array([lo, hi, 0, lo + 1, hi - 1, -1, 1], np.int64)
    assert form_used(ctx, lambda: check(ctx, p, None, s, None, False)) == {"bitmap": 0, "hash": 1}
    check(ctx, p, None, s[:2], None, True)


@pytest.mark.gpu
def test_hash_5000_distinct_sparse_keys(ctx):
    rng = np.random.default_rng(7)
    s = np.unique(rng.integers(-(1 << 62), 1 << 62, 5200).astype(np.int64))[:5000]
    assert len(s) == 5000
    p = np.concatenate([rng.permutation(s)[:3000], rng.integers(-(1 << 62), 1 << 62, 3000).astype(np.int64)])
    used = form_used(ctx, lambda: check(ctx, p, None, s, None, False))
    assert used == {"bitmap": 0, "hash": 1}
    check(ctx, p, rng.random(len(p)) > 0.2, s, rng.random(5000) > 0.01, True, 2, 1)


@pytest.mark.gpu
def test_forced_bitmap_over_a_range_that_cannot_fit_is_an_error(ctx, monkeypatch):
    monkeypatch.setenv("QEH_IN_SET", "bitmap")
    with pytest.raises(qe_hip.QehError) as e:
        ctx.in_set(ctx.upload(np.arange(4, dtype=np.int64)), ctx.upload(np.array([0, 1 << 40], np.int64)))
    assert e.value.status == abi.QEH_E_INVALID


@pytest.mark.gpu
@pytest.mark.parametrize("form", [None, "bitmap", "hash"])
@pytest.mark.parametrize("pt,st", [(np.int32, np.int64), (np.int64, np.int32), (np.int32, np.int32)])
def test_integer_widths_mix(ctx, monkeypatch, form, pt, st):
    if form:
        monkeypatch.setenv("QEH_IN_SET", form)
    rng = np.random.default_rng(3)
    p = rng.integers(-300, 300, 777).astype(pt)
    s = rng.integers(-200, 200, 150).astype(st)
    if st == np.int64 and form != "bitmap":
        s[:2] = [(1 << 32) + 5, -(1 << 32) - 5]  # equal to 5 / -5 in their low 32 bits only
    for negated in (False, True):
        check(ctx, p, rng.random(777) > 0.1, s, None, negated, 1, 3)


@pytest.mark.gpu
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_floats_compare_by_value_bits(ctx, dt):
    it = np.int64 if dt == np.float64 else np.int32
    nan2 = np.array([np.nan], dt).view(it) | 1  # a NaN with other bits
    s = np.array([np.nan, 0.0, 1.5, np.inf], dt)
    p = np.concatenate([np.array([np.nan, -0.0, 0.0, 1.5, 2.0, -np.inf, np.inf], dt), nan2.view(dt)])
    want = [True, False, True, True, False, False, True, False]  # same-bits NaN matches; -0.0 is not 0.0
    vals, valid = run_in_set(ctx, ctx.upload(p), ctx.upload(s), False)
    assert valid.all() and vals.tolist() == want
    for negated in (False, True):
        check(ctx, p, np.arange(8) != 3, s, [True, True, False, True], negated, 3, 1)
        check(ctx, np.tile(p, 40), None, np.array([-0.0], dt), None, negated)


@pytest.mark.gpu
@pytest.mark.parametrize("form", [None, "hash"])
def test_utf8_through_the_shared_dictionary(ctx, monkeypatch, form):
    if form:
        monkeypatch.setenv("QEH_IN_SET", form)
    s = ["", "a", None, "abc", "a", "key-12345678", None]
    p = ["a", "", "b", None, "abc", "ab", "key-12345678", "key-1234567", None, "A"] * 13
    sc = ctx.upload(s)
    pc = ctx.slice(ctx.upload(p), 3, len(p) - 5)  # an offset that is no multiple of 8
    pk = p[3:len(p) - 2]
    for negated in (False, True):
        vals, valid = run_in_set(ctx, pc, sc, negated)
        wv, wm = rule(key_bits(np.array(pk, object)), [x is not None for x in pk],
                      key_bits(np.array(s, object)), [x is not None for x in s], negated)
        assert np.array_equal(valid, wm) and np.array_equal(vals[valid], wv[wm])
    # no NULL in the set: absent strings are decided; an empty-string-only set
    vals, valid = run_in_set(ctx, ctx.upload(p), ctx.upload(["", "zz"]), True)
    wv, wm = rule(key_bits(np.array(p, object)), [x is not None for x in p], [b"", b"zz"], [True, True], True)
    assert np.array_equal(valid, wm) and np.array_equal(vals[valid], wv[wm])


@pytest.mark.gpu
def test_mismatched_types_are_a_type_error(ctx):
    with pytest.raises(qe_hip.QehError) as e:
        ctx.in_set(ctx.upload(np.arange(3, dtype=np.int64)), ctx.upload(["a"]))
    assert e.value.status == abi.QEH_E_TYPE
    assert "Invalid comparison operation: Int64 == Utf8" in e.value.message
    with pytest.raises(qe_hip.QehError) as e:
        ctx.in_set(ctx.upload(np.arange(3, dtype=np.float64)), ctx.upload(np.arange(3, dtype=np.int64)))
    assert e.value.status == abi.QEH_E_TYPE and "Float64 == Int64" in e.value.message


@pytest.mark.gpu
def test_subquery_kinds_are_refused_by_the_operator_entry_points(ctx):
    lib = qe_hip.load()
    arr = (abi.QehExprNode * 1)(abi.QehExprNode(kind=abi.EX_EXISTS, index=0))
    e = abi.QehExpr(arr, 1)
    c = ctx.upload(np.arange(4, dtype=np.int64))
    out = abi.QehColumn()
    assert lib.qeh_eval(ctx.h, abi.C.byref(c.c), 1, abi.C.byref(e), 4, abi.C.byref(out)) == abi.QEH_E_UNSUPPORTED
    assert b"outside a plan" in lib.qeh_last_error()


@pytest.mark.gpu
@pytest.mark.parametrize("n", [6, 2048, 2049])
def test_filter_on_a_literal_alone_keeps_exactly_the_rows_there_are(ctx, n):
    # what EXISTS becomes: a predicate that reads no column must still stop at the last row of a partial tile
    c = ctx.upload(np.arange(n, dtype=np.int64))
    for value, want in [(True, n), (False, 0)]:
        out, rows = ctx.filter([c], lit(value))
        assert rows == want and len(out[0]) == want
        assert np.array_equal(out[0].to_numpy()[0], np.arange(want))
    out, rows = ctx.filter([c], lit(True) & lit(True), max_rows=5)
    assert rows == 5 and np.array_equal(out[0].to_numpy()[0], np.arange(5))


# ---- GPU: plans over employees x departments -----------------------------------------------------

ID, NAME, AGE, SALARY, DEPT = range(5)


@pytest.fixture(scope="module")
def srcs():
    emp = pacsv.read_csv(os.path.join(GOLD, "employees.csv"))  # "NULL" is read as a NULL
    dep = pacsv.read_csv(os.path.join(GOLD, "departments.csv"))
    assert emp["dept_id"].null_count == 1
    return (MemoryDataSource(emp.schema, emp.to_batches()), MemoryDataSource(dep.schema, dep.to_batches()))


def names(batches, column=0):
    return [v for b in batches for v in b.column(column).to_pylist()]


def depts_above(dep, k):
    """SELECT dept_id FROM departments WHERE dept_id > k"""
    return Projection(Filter(Scan(dep), binop(col(0), BinaryOp.Greater, lit(k))), [col(0)], ["dept_id"])


def select_names(emp, pred):
    return Projection(Filter(Scan(emp), pred), [col(NAME)], ["name"])


@pytest.mark.gpu
def test_plan_in_and_not_in(ctx, srcs):
    emp, dep = srcs
    ex = QueryExecutor(ctx)
    sub = depts_above(dep, 101)  # {102, 103, 104}
    assert names(ex.execute(select_names(emp, InSubquery(col(DEPT), sub)))) == ["Bob", "Diana", "Eve"]
    # NOT IN: Frank's NULL dept_id is neither in nor out, so he is dropped
    assert names(ex.execute(select_names(emp, InSubquery(col(DEPT), sub, negated=True)))) == ["Alice", "Charlie"]
    # the unprojected filter keeps every column and the input order
    got = ex.execute(Filter(Scan(emp), InSubquery(col(DEPT), sub)))
    assert names(got, ID) == [2, 4, 5] and names(got, DEPT) == [102, 103, 102]
    # a tested expression that is not a bare column: dept_id + 1 IN {102, 103, 104} -> 101, 102, 103
    plus1 = InSubquery(binop(col(DEPT), BinaryOp.Add, lit(1)), sub)
    assert names(ex.execute(select_names(emp, plus1))) == ["Alice", "Bob", "Charlie", "Diana", "Eve"]


@pytest.mark.gpu
def test_plan_not_in_over_a_subquery_with_a_null_gives_no_rows(ctx, srcs):
    emp, _ = srcs
    sub = Projection(Scan(emp), [col(DEPT)], ["dept_id"])  # 101, 102, 103 and Frank's NULL
    ex = QueryExecutor(ctx)
    assert ex.execute(select_names(emp, InSubquery(col(ID), sub, negated=True))) == []
    # ... while IN still finds what is there: nobody's id is a department
    assert ex.execute(select_names(emp, InSubquery(col(ID), sub))) == []
    assert names(ex.execute(select_names(emp, InSubquery(col(DEPT), sub)))) == ["Alice", "Bob", "Charlie", "Diana", "Eve"]


@pytest.mark.gpu
def test_plan_in_combined_with_and_or_not(ctx, srcs):
    emp, dep = srcs
    ex = QueryExecutor(ctx)
    isin = InSubquery(col(DEPT), depts_above(dep, 101))  # Bob, Diana, Eve; NULL for Frank
    rich = binop(col(SALARY), BinaryOp.Greater, lit(80000))  # Bob, Charlie, Eve
    assert names(ex.execute(select_names(emp, isin & rich))) == ["Bob", "Eve"]
    assert names(ex.execute(select_names(emp, isin | binop(col(SALARY), BinaryOp.Greater, lit(90000))))) == \
        ["Bob", "Charlie", "Diana", "Eve"]
    # NOT (x IN ...): NULL stays NULL, so Frank is still out.  So he is under OR with a TRUE term: the
    # reference's OR is arrow's `or` (operators.rs:540-571), NULL when either side is, not Kleene's
    assert names(ex.execute(select_names(emp, UnaryExpr(UnaryOp.Not, isin)))) == ["Alice", "Charlie"]
    assert names(ex.execute(select_names(emp, isin | binop(col(AGE), BinaryOp.Equal, lit(29))))) == \
        ["Bob", "Diana", "Eve"]


@pytest.mark.gpu
def test_plan_in_as_a_projection_is_a_nullable_boolean(ctx, srcs):
    emp, dep = srcs
    plan = Projection(Scan(emp), [col(NAME), InSubquery(col(DEPT), depts_above(dep, 101)),
                                  InSubquery(col(DEPT), depts_above(dep, 101), negated=True)], ["name", "in", "not_in"])
    (b,) = QueryExecutor(ctx).execute(plan)
    assert str(b.schema.field(1).type) == "bool"
    assert b.column(1).to_pylist() == [False, True, False, True, True, None]
    assert b.column(2).to_pylist() == [True, False, True, False, False, None]


@pytest.mark.gpu
def test_plan_limit_projection_filter_in_equals_the_unfused_plan(ctx, srcs, monkeypatch):
    emp, dep = srcs
    plan = Limit(select_names(emp, InSubquery(col(DEPT), depts_above(dep, 101))), 1, 1)
    fused = names(QueryExecutor(ctx).execute(plan))
    monkeypatch.setenv("QEH_NO_FUSION", "1")
    assert fused == names(QueryExecutor(ctx).execute(plan)) == ["Diana"]


@pytest.mark.gpu
def test_plan_in_under_a_fused_filter_aggregate(ctx, srcs, monkeypatch):
    emp, dep = srcs
    plan = HashAggregate(Filter(Scan(emp), InSubquery(col(DEPT), depts_above(dep, 101))), [col(DEPT)],
                         [AggregateExpr(AF.Sum, col(SALARY))])
    want = [(102, 175000), (103, 80000)]
    (b,) = QueryExecutor(ctx).execute(plan)
    assert sorted(zip(b.column(0).to_pylist(), b.column(1).to_pylist())) == want
    monkeypatch.setenv("QEH_NO_FUSION", "1")
    (b,) = QueryExecutor(ctx).execute(plan)
    assert sorted(zip(b.column(0).to_pylist(), b.column(1).to_pylist())) == want


@pytest.mark.gpu
def test_plan_exists_and_not_exists(ctx, srcs):
    emp, dep = srcs
    ex = QueryExecutor(ctx)
    everyone = ["Alice", "Bob", "Charlie", "Diana", "Eve", "Frank"]
    some, none = depts_above(dep, 101), depts_above(dep, 1000)
    assert names(ex.execute(select_names(emp, Exists(some)))) == everyone
    assert ex.execute(select_names(emp, Exists(some, negated=True))) == []
    assert ex.execute(select_names(emp, Exists(none))) == []
    assert names(ex.execute(select_names(emp, Exists(none, negated=True)))) == everyone
    # combined with a term over the rows
    old = binop(col(AGE), BinaryOp.GreaterEqual, lit(30))
    assert names(ex.execute(select_names(emp, Exists(some) & old))) == ["Bob", "Charlie", "Eve"]


@pytest.mark.gpu
def test_plan_scalar_subquery(ctx, srcs):
    emp, dep = srcs
    ex = QueryExecutor(ctx)
    avg = HashAggregate(Scan(emp), [], [AggregateExpr(AF.Avg, col(SALARY))])  # 83833.33
    above = binop(col(SALARY), BinaryOp.Greater, ScalarSubquery(avg))
    assert names(ex.execute(select_names(emp, above))) == ["Bob", "Charlie", "Eve"]
    # an Int64 scalar: dept_id = (SELECT MAX(dept_id) FROM departments WHERE dept_id < 103)
    mx = HashAggregate(Filter(Scan(dep), binop(col(0), BinaryOp.Less, lit(103))), [], [AggregateExpr(AF.Max, col(0))])
    assert names(ex.execute(select_names(emp, binop(col(DEPT), BinaryOp.Equal, ScalarSubquery(mx))))) == ["Bob", "Eve"]
    # a Utf8 scalar: name = (SELECT manager ...) has no match, name < it has
    who = Projection(Filter(Scan(dep), binop(col(0), BinaryOp.Equal, lit(104))), [col(3)], ["manager"])  # Robert
    assert ex.execute(select_names(emp, binop(col(NAME), BinaryOp.Equal, ScalarSubquery(who)))) == []
    assert names(ex.execute(select_names(emp, binop(col(NAME), BinaryOp.Greater, ScalarSubquery(who))))) == []
    assert names(ex.execute(select_names(emp, binop(col(NAME), BinaryOp.Less, ScalarSubquery(who)))))[-1] == "Frank"


@pytest.mark.gpu
def test_plan_scalar_subquery_over_zero_batches_is_null(ctx, srcs):
    emp, _ = srcs
    ex = QueryExecutor(ctx)
    # the filter keeps nobody, so the global aggregate sees no batch and returns no row (executor.rs:178)
    nobody = Filter(Scan(emp), binop(col(SALARY), BinaryOp.Greater, lit(10 ** 9)))
    avg = HashAggregate(nobody, [], [AggregateExpr(AF.Avg, col(SALARY))])
    assert ex.execute(avg) == []
    assert ex.execute(select_names(emp, binop(col(SALARY), BinaryOp.Greater, ScalarSubquery(avg)))) == []
    assert ex.execute(select_names(emp, binop(col(SALARY), BinaryOp.LessEqual, ScalarSubquery(avg)))) == []
    # zero rows with a schema: a typed NULL as well
    none = Projection(nobody, [col(SALARY)], ["salary"])
    assert ex.execute(select_names(emp, binop(col(SALARY), BinaryOp.NotEqual, ScalarSubquery(none)))) == []
    (b,) = ex.execute(Projection(Scan(emp), [binop(col(SALARY), BinaryOp.Greater, ScalarSubquery(avg))], ["x"]))
    assert b.column(0).to_pylist() == [None] * 6


@pytest.mark.gpu
def test_plan_subquery_errors(ctx, srcs):
    emp, dep = srcs
    ex = QueryExecutor(ctx)
    two_rows = Projection(Scan(dep), [col(0)], ["dept_id"])
    with pytest.raises(qe_hip.QehError) as e:
        ex.execute(select_names(emp, binop(col(DEPT), BinaryOp.Equal, ScalarSubquery(two_rows))))
    assert e.value.status == abi.QEH_E_INVALID and "Scalar subquery returned more than one row" in e.value.message
    with pytest.raises(qe_hip.QehError) as e:
        two_cols = Projection(Scan(dep), [col(0), col(1)], ["dept_id", "dept_name"])
        ex.execute(select_names(emp, InSubquery(col(DEPT), two_cols)))
    assert e.value.status == abi.QEH_E_INVALID and "IN subquery must return exactly one column" in e.value.message
    on = binop(col(DEPT), BinaryOp.Equal, col(5)) & InSubquery(col(DEPT), depts_above(dep, 101))
    with pytest.raises(qe_hip.QehError) as e:
        ex.execute(HashJoin(Scan(emp), Scan(dep), JoinType.Inner, on))
    assert e.value.status == abi.QEH_E_UNSUPPORTED and "join condition" in e.value.message
    with pytest.raises(qe_hip.QehError) as e:
        ex.execute(HashAggregate(Scan(emp), [], [AggregateExpr(AF.Sum, ScalarSubquery(two_rows))]))
    assert e.value.status == abi.QEH_E_UNSUPPORTED and "aggregate argument" in e.value.message
    # Int64 dept_id against a Utf8 subquery column: arrow's comparison error
    with pytest.raises(qe_hip.QehError) as e:
        ex.execute(select_names(emp, InSubquery(col(DEPT), Projection(Scan(dep), [col(1)], ["dept_name"]))))
    assert e.value.status == abi.QEH_E_TYPE and "Int64 == Utf8" in e.value.message


@pytest.mark.gpu
def test_plan_two_subqueries_in_one_predicate(ctx, srcs):
    emp, dep = srcs
    sub = depts_above(dep, 101)
    # id NOT IN {102, 103, 104} is TRUE for all six; Frank's NULL IN (...) makes his OR NULL (arrow's
    # `or`, operators.rs:540-571, is NULL when either side is), so he alone is dropped
    plan = select_names(emp, InSubquery(col(DEPT), sub) | InSubquery(col(ID), sub, negated=True))
    assert names(QueryExecutor(ctx).execute(plan)) == ["Alice", "Bob", "Charlie", "Diana", "Eve"]
    # ... and under AND he is dropped again
    plan = select_names(emp, InSubquery(col(DEPT), sub, negated=True) & InSubquery(col(ID), sub, negated=True))
    assert names(QueryExecutor(ctx).execute(plan)) == ["Alice", "Charlie"]
