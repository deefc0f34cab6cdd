"""Date32, Date64 and Timestamp columns on the device: import / export keep the Arrow DataType,
comparisons and keys run on the physical integers with arrow's semantics, the operators the
reference refuses are refused with its messages, and qeh_encode_pg_datarows renders the cells as
the reference's pgwire front end does (tests/temporal_text.py).  Checkers: pyarrow and Python."""
import ctypes

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pytest

import qe_hip
import temporal_text as tt
from qe_hip import (AggregateExpr, AggregateFunction as AF, BinaryOp, Filter, HashAggregate, HashJoin, InSubquery,
                    JoinType, Limit, MemoryDataSource, Projection, QehError, QueryExecutor, ScalarFunction,
                    ScalarFunctionType as FN, Scan, Sort, UnaryExpr, UnaryOp, Window, WindowExpr, WindowFunctionType,
                    abi, binop, col, lit)
from qe_hip.expr import Column

# name in tests/temporal_text.py, Arrow type, qeh dtype, physical Arrow type
TYPES = [("date32", pa.date32(), abi.DT_DATE32, pa.int32()),
         ("date64", pa.date64(), abi.DT_DATE64, pa.int64()),
         ("ts_s", pa.timestamp("s"), abi.DT_TIMESTAMP_S, pa.int64()),
         ("ts_ms", pa.timestamp("ms"), abi.DT_TIMESTAMP_MS, pa.int64()),
         ("ts_us", pa.timestamp("us"), abi.DT_TIMESTAMP_US, pa.int64()),
         ("ts_ns", pa.timestamp("ns"), abi.DT_TIMESTAMP_NS, pa.int64())]
ARROW_NAME = {abi.DT_DATE32: "Date32", abi.DT_DATE64: "Date64", abi.DT_TIMESTAMP_S: "Timestamp(Second, None)",
              abi.DT_TIMESTAMP_MS: "Timestamp(Millisecond, None)", abi.DT_TIMESTAMP_US: "Timestamp(Microsecond, None)",
              abi.DT_TIMESTAMP_NS: "Timestamp(Nanosecond, None)", abi.DT_INT64: "Int64", abi.DT_INT32: "Int32"}
DAY_MIN, DAY_MAX = -719528, 2932896  # 0000-01-01 .. 9999-12-31
CMP = "Invalid argument error: Invalid comparison operation: "


def temporal(ints, valid, typ, phys):
    """pyarrow array of `typ` over the physical integers (None: no NULLs)."""
    a = pa.array(np.asarray(ints), type=phys, mask=None if valid is None else ~np.asarray(valid, bool))
    return a.view(typ)


def ints_of(arr):
    """[int | None] of a temporal pyarrow (chunked) array: its physical integers."""
    if isinstance(arr, pa.ChunkedArray):
        arr = arr.combine_chunks()
    phys = pa.int32() if arr.type == pa.date32() else pa.int64()
    return arr.view(phys).to_pylist() if arr.type != phys else arr.to_pylist()


def source(table: pa.Table):
    return MemoryDataSource(table.schema, table.to_batches())


@pytest.fixture(scope="module")
def qx(ctx):
    return QueryExecutor(ctx)


# ---- 1. round trip -------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name,typ,dt,phys", TYPES, ids=[t[0] for t in TYPES])
def test_round_trip_keeps_the_arrow_type(ctx, qx, name, typ, dt, phys):
    """Scan -> Projection(col) -> result, qeh_encode_arrow_ipc -> pyarrow, pyarrow -> qeh_decode_arrow_ipc:
    the same DataType and values, with NULLs and a non-zero Arrow offset."""
    r = np.random.default_rng(dt)
    n = 50
    lim = 2 ** 31 - 1 if phys == pa.int32() else 2 ** 62
    full = temporal(r.integers(-lim, lim, n + 7), r.random(n + 7) > 0.2, typ, phys)
    arr = full.slice(5, n)
    assert arr.offset == 5 and arr.null_count > 0
    t = pa.Table.from_arrays([arr, pa.array(np.arange(n))], names=["t.c", "t.i"])
    out = qx.execute(Projection(Scan(source(t)), [Column("t.c", 0)], ["t.c"]))
    assert len(out) == 1 and out[0].schema.field(0).type == typ
    assert ints_of(out[0].column(0)) == ints_of(arr)
    # the device column <-> pyarrow
    dcol = ctx.upload_arrow(arr, offset=3)
    assert dcol.dtype == dt and dcol.to_arrow().type == typ and ints_of(dcol.to_arrow()) == ints_of(arr)
    # our IPC writer -> pyarrow's reader
    got = pa.ipc.open_stream(pa.py_buffer(ctx.encode_arrow_ipc([dcol], ["c"]))).read_all()
    assert got.schema.field(0).type == typ and got.schema.names == ["c"]
    assert ints_of(got.column(0)) == ints_of(arr)
    # pyarrow's writer -> our IPC reader
    sink = pa.BufferOutputStream()
    tb = pa.Table.from_arrays([arr], names=["c"])
    with pa.ipc.new_stream(sink, tb.schema) as w:
        w.write_table(tb)
    names, cols, rows = ctx.decode_arrow_ipc(sink.getvalue().to_pybytes())
    assert names == ["c"] and rows == n and cols[0].dtype == dt
    assert cols[0].to_arrow().type == typ and ints_of(cols[0].to_arrow()) == ints_of(arr)


@pytest.mark.gpu
def test_numpy_datetime64_upload_and_download(ctx):
    days = np.array(["1970-01-01", "2000-02-29", "1969-12-31"], "datetime64[D]")
    c = ctx.upload(days)
    assert c.dtype == abi.DT_DATE32
    v, _ = c.to_numpy()
    assert v.dtype == np.dtype("datetime64[D]") and np.array_equal(v, days)
    us = np.array([1, -1, 1_500_000], np.int64)
    c = ctx.upload(us.view("datetime64[us]"))
    assert c.dtype == abi.DT_TIMESTAMP_US and np.array_equal(c.to_numpy()[0].view(np.int64), us)
    c = ctx.upload(us, dtype=abi.DT_DATE64)
    assert c.dtype == abi.DT_DATE64 and c.to_arrow().type == pa.date64()


# ---- 2. a temporal column the query never reads ---------------------------------------------------

@pytest.mark.gpu
def test_filter_over_a_table_with_an_unrelated_timestamp_column(qx):
    r = np.random.default_rng(2)
    n = 3000
    t = pa.table({"orders.id": np.arange(n), "orders.amount": r.integers(0, 20, n),
                  "orders.created_at": temporal(r.integers(0, 2 ** 50, n), r.random(n) > 0.1, pa.timestamp("us"), pa.int64())})
    plan = Projection(Filter(Scan(source(t)), binop(Column("orders.amount", 1), BinaryOp.Greater, lit(10))),
                      [Column("orders.id", 0)], ["orders.id"])
    out = qx.execute(plan)
    want = t.filter(pc.greater(t["orders.amount"], 10))["orders.id"].to_pylist()
    assert pa.Table.from_batches(out)["orders.id"].to_pylist() == want
    # ... and with the column carried along
    out = qx.execute(Filter(Scan(source(t)), binop(Column("orders.amount", 1), BinaryOp.Greater, lit(10))))
    got = pa.Table.from_batches(out)
    assert got.schema.field(2).type == pa.timestamp("us")
    assert ints_of(got.column(2)) == ints_of(t.filter(pc.greater(t["orders.amount"], 10)).column(2))


# ---- 3. typing (host only) ------------------------------------------------------------------------

def ty(expr, dtypes):
    lib = qe_hip.load()
    e, keep = expr.to_c()
    d = (ctypes.c_int32 * len(dtypes))(*dtypes)
    out = ctypes.c_int32()
    s = lib.qeh_expr_type(d, len(dtypes), ctypes.byref(e), ctypes.byref(out))
    return s, out.value, lib.qeh_last_error().decode()


CMP_OPS = [(BinaryOp.Equal, "=="), (BinaryOp.NotEqual, "!="), (BinaryOp.Less, "<"), (BinaryOp.LessEqual, "<="),
           (BinaryOp.Greater, ">"), (BinaryOp.GreaterEqual, ">=")]


def test_same_type_comparisons_type_to_boolean():
    for _, _, dt, _ in TYPES:
        for op, _ in CMP_OPS:
            assert ty(binop(col(0), op, col(1)), [dt, dt])[:2] == (0, abi.DT_BOOL), (dt, op)


def test_comparisons_with_any_other_type_are_arrow_errors():
    D32, D64, US, MS = abi.DT_DATE32, abi.DT_DATE64, abi.DT_TIMESTAMP_US, abi.DT_TIMESTAMP_MS
    for op, sym in CMP_OPS:
        s, _, msg = ty(binop(col(0), op, col(1)), [D32, abi.DT_INT64])
        assert s == abi.QEH_E_TYPE and msg == f"{CMP}Date32 {sym} Int64"
    for lt, rt in [(D32, D64), (D32, abi.DT_INT32), (D64, abi.DT_INT64), (US, abi.DT_INT64), (abi.DT_INT64, US),
                   (US, MS), (abi.DT_TIMESTAMP_S, abi.DT_TIMESTAMP_NS), (D64, MS)]:
        s, _, msg = ty(binop(col(0), BinaryOp.Equal, col(1)), [lt, rt])
        assert s == abi.QEH_E_TYPE and msg == f"{CMP}{ARROW_NAME[lt]} == {ARROW_NAME[rt]}", (lt, rt, msg)
    s, _, msg = ty(binop(col(0), BinaryOp.Less, col(1)), [US, MS])
    assert msg.startswith(CMP) and msg == CMP + "Timestamp(Microsecond, None) < Timestamp(Millisecond, None)"
    # there are no temporal literals: an integer literal is an Int64 array
    s, _, msg = ty(binop(col(0), BinaryOp.Greater, lit(10)), [D32])
    assert s == abi.QEH_E_TYPE and msg == f"{CMP}Date32 > Int64"
    s, _, msg = ty(binop(col(0), BinaryOp.Equal, lit(None)), [US])
    assert s == abi.QEH_E_TYPE and msg == f"{CMP}Timestamp(Microsecond, None) == Null"


def test_other_operators_and_functions_refuse_temporal_operands():
    for _, _, dt, _ in TYPES:
        for op, word in [(BinaryOp.Add, "addition"), (BinaryOp.Subtract, "subtraction"),
                         (BinaryOp.Multiply, "multiplication"), (BinaryOp.Divide, "division")]:
            s, _, msg = ty(binop(col(0), op, col(1)), [dt, dt])
            assert s == abi.QEH_E_TYPE and msg == f"Unsupported types for {word}", (dt, word)
        s, _, msg = ty(binop(col(0), BinaryOp.Modulo, col(1)), [dt, dt])
        assert s == abi.QEH_E_TYPE and msg == "Modulo operation requires integer arrays"
        s, _, msg = ty(UnaryExpr(UnaryOp.Minus, col(0)), [dt])
        assert s == abi.QEH_E_TYPE and msg == "Unsupported type for negation"
        s, _, msg = ty(UnaryExpr(UnaryOp.Not, col(0)), [dt])
        assert s == abi.QEH_E_TYPE and msg == "NOT operator requires boolean array"
        s, _, msg = ty(binop(col(0), BinaryOp.And, col(1)), [dt, abi.DT_BOOL])
        assert s == abi.QEH_E_TYPE and msg == "AND requires boolean arrays"
        s, _, msg = ty(binop(col(1), BinaryOp.Or, col(0)), [dt, abi.DT_BOOL])
        assert s == abi.QEH_E_TYPE and msg == "OR requires boolean arrays"
        for fn, text in [(FN.Upper, "UPPER requires string argument"), (FN.Length, "LENGTH requires string argument"),
                         (FN.Abs, "ABS requires numeric argument"), (FN.Ceil, "CEIL requires float argument"),
                         (FN.Sqrt, "SQRT requires float argument"), (FN.Concat, "CONCAT requires string arguments")]:
            s, _, msg = ty(ScalarFunction(fn, [col(0)]), [dt])
            assert s == abi.QEH_E_TYPE and msg == text, (dt, text)
        assert ty(ScalarFunction(FN.Coalesce, [col(0), col(1)]), [dt, abi.DT_INT64])[:2] == (0, dt)


# ---- 4. comparisons on the device -------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["date32", "ts_us"])
def test_column_comparisons_match_pyarrow(ctx, name):
    _, typ, dt, phys = next(t for t in TYPES if t[0] == name)
    r = np.random.default_rng(dt + 40)
    n = 1000
    lo, hi = (DAY_MIN, DAY_MAX) if name == "date32" else (DAY_MIN * 86400 * 10 ** 6, (DAY_MAX + 1) * 86400 * 10 ** 6 - 1)
    pool = np.concatenate([[lo, hi, 0, -1, 1], r.integers(lo, hi, 20)])
    a, b = pool[r.integers(0, len(pool), n)], pool[r.integers(0, len(pool), n)]
    va, vb = r.random(n) > 0.1, r.random(n) > 0.1
    pa_a, pa_b = temporal(a, va, typ, phys), temporal(b, vb, typ, phys)
    da, db = ctx.upload_arrow(pa_a), ctx.upload_arrow(pa_b, offset=5)
    fns = [pc.equal, pc.not_equal, pc.less, pc.less_equal, pc.greater, pc.greater_equal]
    for (op, _), fn in zip(CMP_OPS, fns):
        got = ctx.eval([da, db], binop(col(0), op, col(1)))
        assert got.dtype == abi.DT_BOOL
        assert got.to_arrow().to_pylist() == fn(pa_a, pa_b).to_pylist(), op
    # COALESCE hands its first argument back unchanged
    same, _src = ctx.eval([da, db], ScalarFunction(FN.Coalesce, [col(0), col(1)]))  # a view of `da`
    assert same.dtype == dt and ints_of(same.to_arrow()) == ints_of(pa_a)


# ---- 5. keys --------------------------------------------------------------------------------------------

N_KEYS = 5000


@pytest.fixture(scope="module")
def keyed():
    """5000 rows: a Date32 and a Timestamp(us) key of ~200 distinct values on both sides of the
    epoch with ~5 % NULLs, an Int64 partition key and a unique Int64 value."""
    r = np.random.default_rng(77)
    dpool = np.unique(r.integers(-200_000, 200_000, 200)).astype(np.int32)
    upool = np.unique(r.integers(-10 ** 15, 10 ** 15, 200))
    d = dpool[r.integers(0, len(dpool), N_KEYS)]
    u = upool[r.integers(0, len(upool), N_KEYS)]
    vd, vu = r.random(N_KEYS) > 0.05, r.random(N_KEYS) > 0.05
    return {"d": temporal(d, vd, pa.date32(), pa.int32()), "u": temporal(u, vu, pa.timestamp("us"), pa.int64()),
            "p": pa.array(r.integers(0, 7, N_KEYS)), "v": pa.array(np.arange(N_KEYS)), "dpool": dpool}


def want_order(arr, asc, nulls_first=True):
    """qeh_sort_indices' documented order: NULLs first (or last), ties by input position."""
    t = pa.table({"k": arr})
    return pc.sort_indices(t, sort_keys=[("k", "ascending" if asc else "descending")],
                           null_placement="at_start" if nulls_first else "at_end").to_pylist()


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["d", "u"])
@pytest.mark.parametrize("asc", [True, False])
def test_order_by_a_temporal_key(ctx, qx, keyed, key, asc):
    arr = keyed[key]
    dk = ctx.upload_arrow(arr)
    want = want_order(arr, asc)
    assert ctx.sort_indices([dk], [asc]).to_numpy()[0].tolist() == want
    assert ctx.sort_indices_nulls([dk], [asc], [False]).to_numpy()[0].tolist() == want_order(arr, asc, False)
    assert ctx.sort_indices_limit([dk], [asc], 10).to_numpy()[0].tolist() == want[:10]
    # through a plan: Sort, and Limit(Sort) with k = 10; the key keeps its type
    t = pa.table({"t.k": arr, "t.v": keyed["v"]})
    plan = Sort(Scan(source(t)), [Column("t.k", 0)], [asc])
    got = pa.Table.from_batches(qx.execute(plan))
    assert got.schema.field(0).type == arr.type
    assert got["t.v"].to_pylist() == want and ints_of(got["t.k"]) == ints_of(arr.take(pa.array(want)))
    top = pa.Table.from_batches(qx.execute(Limit(plan, 0, 10)))
    assert top["t.v"].to_pylist() == want[:10] and top.schema.field(0).type == arr.type


def group_counts(table, key, val):
    g = table.group_by(key).aggregate([(val, "count")])
    return sorted(zip(ints_of(g[key]), g[f"{val}_count"].to_pylist()), key=lambda kv: (kv[0] is not None, kv[0] or 0))


@pytest.mark.gpu
@pytest.mark.parametrize("key", ["d", "u"])
@pytest.mark.parametrize("fused", [True, False])
def test_group_by_a_temporal_key_with_count(qx, keyed, monkeypatch, key, fused):
    if not fused:
        monkeypatch.setenv("QEH_NO_FUSION", "1")
    t = pa.table({"t.k": keyed[key], "t.v": keyed["v"], "t.p": keyed["p"]})
    aggs = [AggregateExpr(AF.Count, Column("t.v", 1))]
    got = pa.Table.from_batches(qx.execute(HashAggregate(Scan(source(t)), [Column("t.k", 0)], aggs)))
    assert got.schema.field(0).type == keyed[key].type and got.schema.names == ["t.k", "col_0"]
    rows = sorted(zip(ints_of(got["t.k"]), got["col_0"].to_pylist()), key=lambda kv: (kv[0] is not None, kv[0] or 0))
    assert rows == group_counts(t, "t.k", "t.v")
    # HashAggregate(Filter(X)): the fused filter-aggregate, or the chain
    pred = binop(Column("t.p", 2), BinaryOp.Greater, lit(2))
    got = pa.Table.from_batches(qx.execute(HashAggregate(Filter(Scan(source(t)), pred), [Column("t.k", 0)], aggs)))
    assert got.schema.field(0).type == keyed[key].type
    rows = sorted(zip(ints_of(got["t.k"]), got["col_0"].to_pylist()), key=lambda kv: (kv[0] is not None, kv[0] or 0))
    assert rows == group_counts(t.filter(pc.greater(t["t.p"], 2)), "t.k", "t.v")


@pytest.fixture(scope="module")
def dim(keyed):
    """300 build rows: unique Date32 keys, two thirds of them from the fact side's pool, a
    Timestamp(us) attribute of 11 distinct values and an Int64 one."""
    r = np.random.default_rng(78)
    keys = np.concatenate([keyed["dpool"][:200], np.arange(300_000, 300_000 + 300 - len(keyed["dpool"][:200]))])
    keys = r.permutation(keys.astype(np.int32))
    g = (r.integers(-5, 6, len(keys)) * 10 ** 9 + 1).astype(np.int64)
    return pa.table({"r.k": temporal(keys, None, pa.date32(), pa.int32()),
                     "r.g": temporal(g, r.random(len(keys)) > 0.1, pa.timestamp("us"), pa.int64()),
                     "r.w": pa.array(np.arange(len(keys)) * 3)})


def row_set(table, names):
    cols = [ints_of(table[n]) if pa.types.is_temporal(table[n].type) else table[n].to_pylist() for n in names]
    return sorted(zip(*cols), key=lambda row: tuple((x is not None, x or 0) for x in row))


@pytest.mark.gpu
@pytest.mark.parametrize("jt,pa_jt", [(JoinType.Inner, "inner"), (JoinType.Left, "left outer")])
def test_join_on_a_date32_key(qx, keyed, dim, jt, pa_jt):
    left = pa.table({"l.k": keyed["d"], "l.v": keyed["v"]})
    on = binop(Column("l.k", 0), BinaryOp.Equal, Column("r.k", 2))
    got = pa.Table.from_batches(qx.execute(HashJoin(Scan(source(left)), Scan(source(dim)), jt, on)))
    assert got.schema.names == ["l.k", "l.v", "r.k", "r.g", "r.w"]
    assert [f.type for f in got.schema] == [pa.date32(), pa.int64(), pa.date32(), pa.timestamp("us"), pa.int64()]
    want = left.join(dim, keys="l.k", right_keys="r.k", join_type=pa_jt, coalesce_keys=False)
    names = ["l.k", "l.v", "r.k", "r.g", "r.w"]
    assert row_set(got, names) == row_set(want, names)


@pytest.mark.gpu
def test_join_keys_of_different_types_are_a_comparison_error(ctx, qx, keyed, dim):
    d = ctx.upload_arrow(keyed["d"].slice(0, 100))
    i32 = ctx.upload(np.arange(100, dtype=np.int32))
    u = ctx.upload_arrow(keyed["u"].slice(0, 100))
    for a, b, text in [(d, i32, "Date32 == Int32"), (i32, d, "Int32 == Date32"),
                       (d, u, "Date32 == Timestamp(Microsecond, None)")]:
        with pytest.raises(QehError) as e:
            ctx.hash_join(0, a, [a], b, [b])
        assert e.value.status == abi.QEH_E_TYPE and e.value.message == CMP + text
        with pytest.raises(QehError) as e:
            ctx.in_set(a, b)
        assert e.value.status == abi.QEH_E_TYPE and e.value.message == CMP + text


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [True, False])
def test_join_aggregate_on_temporal_keys(qx, keyed, dim, monkeypatch, fused):
    """HashAggregate(HashJoin) joined on a Date32 key and grouped by a Timestamp(us) column: the
    fused join-aggregate and the unfused chain give the same groups."""
    if not fused:
        monkeypatch.setenv("QEH_NO_FUSION", "1")
    left = pa.table({"l.k": keyed["d"], "l.v": keyed["v"]})
    on = binop(Column("l.k", 0), BinaryOp.Equal, Column("r.k", 2))
    plan = HashAggregate(HashJoin(Scan(source(left)), Scan(source(dim)), JoinType.Inner, on), [Column("r.g", 3)],
                         [AggregateExpr(AF.Count, Column("l.v", 1)), AggregateExpr(AF.Sum, Column("l.v", 1))])
    got = pa.Table.from_batches(qx.execute(plan))
    assert got.schema.field(0).type == pa.timestamp("us") and got.schema.names == ["r.g", "col_0", "col_1"]
    j = left.join(dim, keys="l.k", right_keys="r.k", join_type="inner", coalesce_keys=False)
    w = j.group_by("r.g").aggregate([("l.v", "count"), ("l.v", "sum")])
    assert row_set(got, ["r.g", "col_0", "col_1"]) == row_set(w, ["r.g", "l.v_count", "l.v_sum"])


@pytest.mark.gpu
@pytest.mark.parametrize("set_has_null", [False, True])
def test_in_and_not_in_subquery_over_a_date32_column(qx, keyed, dim, set_has_null):
    t = pa.table({"t.k": keyed["d"], "t.v": keyed["v"]})
    sk = dim["r.k"].combine_chunks().slice(0, 120)
    if set_has_null:
        sk = pa.concat_arrays([sk, pa.array([None], pa.date32())])
    sub = Projection(Scan(source(pa.table({"s.k": sk}))), [Column("s.k", 0)], ["s.k"])
    members = set(x for x in ints_of(sk) if x is not None)
    keys = ints_of(keyed["d"])
    got_in = pa.Table.from_batches(qx.execute(Filter(Scan(source(t)), InSubquery(Column("t.k", 0), sub))))
    assert got_in["t.v"].to_pylist() == [i for i, k in enumerate(keys) if k is not None and k in members]
    assert got_in.schema.field(0).type == pa.date32()
    out = qx.execute(Filter(Scan(source(t)), InSubquery(Column("t.k", 0), sub, negated=True)))
    want = [] if set_has_null else [i for i, k in enumerate(keys) if k is not None and k not in members]
    assert (pa.Table.from_batches(out)["t.v"].to_pylist() if out else []) == want


@pytest.mark.gpu
def test_window_over_a_timestamp_order_key(qx, keyed):
    """ROW_NUMBER and LAG(x, 1) OVER (PARTITION BY p ORDER BY u): LAG of the Timestamp(us) order key and
    of the Date32 column keep their types."""
    t = pa.table({"t.p": keyed["p"], "t.u": keyed["u"], "t.d": keyed["d"]})
    part, order = [Column("t.p", 0)], [Column("t.u", 1)]
    plan = Window(Scan(source(t)),
                  [WindowExpr(WindowFunctionType.RowNumber, [], part, order),
                   WindowExpr(WindowFunctionType.Lag, [Column("t.u", 1), lit(1)], part, order),
                   WindowExpr(WindowFunctionType.Lag, [Column("t.d", 2), lit(1)], part, order)],
                  ["t.p", "t.u", "t.d", "rn", "lag_u", "lag_d"])
    got = pa.Table.from_batches(qx.execute(plan))
    assert got.schema.field("lag_u").type == pa.timestamp("us") and got.schema.field("lag_d").type == pa.date32()
    p, u, d = np.asarray(keyed["p"]), ints_of(keyed["u"]), ints_of(keyed["d"])
    order_rows = sorted(range(N_KEYS), key=lambda i: (p[i], u[i] is not None, u[i] or 0, i))  # NULLs first, ties by position
    rn, lag_u, lag_d = [0] * N_KEYS, [None] * N_KEYS, [None] * N_KEYS
    prev = None
    for i in order_rows:
        first = prev is None or p[prev] != p[i]
        rn[i] = 1 if first else rn[prev] + 1
        if not first:
            lag_u[i], lag_d[i] = u[prev], d[prev]
        prev = i
    assert got["rn"].to_pylist() == rn
    assert ints_of(got["lag_u"]) == lag_u
    assert ints_of(got["lag_d"]) == lag_d


@pytest.mark.gpu
def test_payload_columns_keep_their_type_through_row_movers(ctx, keyed):
    d = ctx.upload_arrow(keyed["d"])
    u = ctx.upload_arrow(keyed["u"].view(pa.int64()).fill_null(0).view(pa.timestamp("us")))  # no NULLs
    idx = ctx.upload(np.arange(N_KEYS - 1, -1, -1, dtype=np.uint32))
    rev = ctx.take(d, idx)
    assert rev.dtype == abi.DT_DATE32 and ints_of(rev.to_arrow()) == ints_of(keyed["d"])[::-1]
    sc = ctx.scatter(u, idx)
    assert sc.dtype == abi.DT_TIMESTAMP_US and ints_of(sc.to_arrow()) == ints_of(u.to_arrow())[::-1]
    cat = ctx.concat([d, rev])
    assert cat.dtype == abi.DT_DATE32 and ints_of(cat.to_arrow()) == ints_of(keyed["d"]) + ints_of(keyed["d"])[::-1]
    # the partition move: an Int64 key, a non-null Timestamp(us) payload and a nullable Date32 one
    key = ctx.upload(np.asarray(keyed["p"]).astype(np.int64))
    counts, moved = ctx.partition_hash_move([key], 4, [u, d, key])
    assert moved[0].dtype == abi.DT_TIMESTAMP_US and moved[1].dtype == abi.DT_DATE32 and counts.sum() == N_KEYS
    got = sorted(zip(moved[2].to_numpy()[0].tolist(), ints_of(moved[0].to_arrow()),
                     [(-1 if x is None else x) for x in ints_of(moved[1].to_arrow())]))
    want = sorted(zip(np.asarray(keyed["p"]).tolist(), ints_of(u.to_arrow()),
                      [(-1 if x is None else x) for x in ints_of(keyed["d"])]))
    assert got == want
    # a merge keyed on the Int64 column carries the temporal payloads along
    out, rows = ctx.merge_sorted([[key, d, u]], [0], [True], [True])
    assert rows == N_KEYS and out[1].dtype == abi.DT_DATE32 and out[2].dtype == abi.DT_TIMESTAMP_US
    perm = np.argsort(np.asarray(keyed["p"]), kind="stable")
    assert ints_of(out[1].to_arrow()) == [ints_of(keyed["d"])[i] for i in perm]


# ---- 6. aggregates -----------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("key", ["d", "u"])
def test_count_works_and_the_other_aggregates_are_type_errors(ctx, keyed, key):
    arr = keyed[key]
    x, p = ctx.upload_arrow(arr), ctx.upload(np.asarray(keyed["p"]).astype(np.int64))
    _, aggs, g = ctx.hash_aggregate([], [x], [(AF.Count, 0)])
    assert g == 1 and aggs[0].to_numpy()[0].tolist() == [N_KEYS - arr.null_count]
    keys, aggs, g = ctx.hash_aggregate([p], [x], [(AF.Count, 0)])
    want = pa.table({"p": keyed["p"], "x": arr}).group_by("p").aggregate([("x", "count")])
    assert sorted(zip(keys[0].to_numpy()[0].tolist(), aggs[0].to_numpy()[0].tolist())) == \
        sorted(zip(want["p"].to_pylist(), want["x_count"].to_pylist()))
    for func, name in [(AF.Sum, "SUM"), (AF.Avg, "AVG"), (AF.Min, "MIN"), (AF.Max, "MAX")]:
        for group_keys in ([], [p]):
            with pytest.raises(QehError) as e:
                ctx.hash_aggregate(group_keys, [x], [(func, 0)])
            assert e.value.status == abi.QEH_E_TYPE and e.value.message == f"Unsupported type for {name}"


# ---- 7. still refused -----------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_partition_and_merge_keys_and_zoned_timestamps_are_refused(ctx, qx, keyed):
    d, u = ctx.upload_arrow(keyed["d"]), ctx.upload_arrow(keyed["u"])
    v = ctx.upload(np.arange(N_KEYS, dtype=np.int64))
    lib = ctx.lib
    counts = (ctypes.c_int64 * 4)()
    out = abi.QehColumn()
    bounds = (ctypes.c_int64 * 3)(-10, 0, 10)
    for k in (d, u):
        assert lib.qeh_partition_hash(ctx.h, ctypes.byref(k.c), 1, 4, counts, ctypes.byref(out)) == abi.QEH_E_UNSUPPORTED
        assert lib.qeh_partition_range(ctx.h, ctypes.byref(k.c), bounds, 3, counts, ctypes.byref(out)) == abi.QEH_E_UNSUPPORTED
        for call in (lambda: ctx.hash_partition(k, 4), lambda: ctx.range_partition(k, [0, 10]),
                     lambda: ctx.partition_hash_move([k], 4, [v]), lambda: ctx.merge_sorted([[k, v]], [0], [True], [True]),
                     lambda: ctx.merge_sorted([[k, v, v]], [0], [True], [True])):
            with pytest.raises(QehError) as e:
                call()
            assert e.value.status == abi.QEH_E_UNSUPPORTED
    zoned = pa.table({"t.z": pa.array([1, 2, 3], pa.timestamp("us", tz="UTC")), "t.i": pa.array([1, 2, 3])})
    with pytest.raises(QehError) as e:
        qx.execute(Projection(Scan(source(zoned)), [Column("t.i", 1)], ["t.i"]))
    assert e.value.status == abi.QEH_E_UNSUPPORTED and "arrow type 'tsu:UTC' is not supported on the device" in e.value.message
    sink = pa.BufferOutputStream()
    with pa.ipc.new_stream(sink, zoned.schema) as w:
        w.write_table(zoned)
    with pytest.raises(QehError) as e:
        ctx.decode_arrow_ipc(sink.getvalue().to_pybytes())
    assert e.value.status == abi.QEH_E_UNSUPPORTED


# ---- 8. pgwire text ---------------------------------------------------------------------------------------------

HAND = {"date32": [0, -1, 11016, DAY_MIN, DAY_MAX],
        "date64": [-1, -1000, -1001, -86400000, -86400001, 0, 999, DAY_MIN * 86400000, DAY_MAX * 86400000 + 86399999],
        "ts_s": [0, -1, DAY_MIN * 86400, DAY_MAX * 86400 + 86399],
        "ts_ms": [1500, -1, 1000, -1500],
        "ts_us": [1, -1, 1_500_000, 1_000_000, -1_000_001],
        "ts_ns": [1, 1000, 1_000_000, -1, 10 ** 9, -(2 ** 63), 2 ** 63 - 1]}


def pg_columns(n, shape, seed):
    """[(text name, values, valid, Arrow type, physical type)]: the six temporal types interleaved with an
    Int64 and a Utf8 column; values random inside years 0000-9999 plus the hand-written ones."""
    r = np.random.default_rng(seed)
    sec_lo, sec_hi = DAY_MIN * 86400, DAY_MAX * 86400 + 86399

    def with_hand(name, vals):
        h = HAND[name][:n]
        vals[:len(h)] = h
        return vals

    def valid(p=0.1):
        v = r.random(n) > p
        v[:min(n, 10)] = True  # the hand-written values stay visible
        return v
    d32 = with_hand("date32", r.integers(DAY_MIN, DAY_MAX + 1, n).astype(np.int32))
    d64 = r.integers(DAY_MIN, DAY_MAX + 1, n) * 86400000 + r.integers(0, 86400000, n)
    d64[n // 2:] = d64[n // 2:] // 1000 * 1000  # half on a multiple of 1000: negatives render, the others are "NULL"
    d64 = with_hand("date64", d64)
    secs = r.integers(sec_lo, sec_hi + 1, n)
    frac = lambda per: np.where(r.random(n) < 0.3, 0, r.integers(0, per, n))  # noqa: E731
    ts_s = with_hand("ts_s", secs.copy())
    ts_ms = with_hand("ts_ms", secs * 1000 + frac(1000))
    ts_us = with_hand("ts_us", secs * 10 ** 6 + np.where(r.random(n) < 0.3, frac(1000) * 1000, frac(10 ** 6)))
    ns = r.integers(-(2 ** 63), 2 ** 63 - 1, n)
    ns = np.where(r.random(n) < 0.5, ns // 1000 * 1000, ns)
    ns = np.where(r.random(n) < 0.3, ns // 10 ** 6 * 10 ** 6, ns)
    ts_ns = with_hand("ts_ns", ns)  # every Int64 nanosecond count lies inside years 1677-2262
    i64 = r.integers(-(2 ** 40), 2 ** 40, n)
    width = {"narrow": 0, "wide": 9, "long": 400}[shape]
    utf8 = np.array([("x" * (i % (width + 1))) if shape != "long" else "y" * (width + i % 7) for i in range(n)], dtype=object)
    if shape == "narrow":
        return [("int64", r.integers(-999, 1000, n), None, pa.int64(), pa.int64()),
                ("date32", d32, valid(), pa.date32(), pa.int32()),
                ("date64", d64, valid(0.5), pa.date64(), pa.int64())]
    return [("date32", d32, valid(), pa.date32(), pa.int32()), ("int64", i64, valid(), pa.int64(), pa.int64()),
            ("date64", d64, valid(), pa.date64(), pa.int64()), ("ts_s", ts_s, valid(), pa.timestamp("s"), pa.int64()),
            ("utf8", utf8, valid(), pa.string(), None), ("ts_ms", ts_ms, None, pa.timestamp("ms"), pa.int64()),
            ("ts_us", ts_us, valid(), pa.timestamp("us"), pa.int64()), ("ts_ns", ts_ns, valid(), pa.timestamp("ns"), pa.int64())]


def upload_pg(ctx, cols):
    dev = []
    for name, vals, valid, typ, phys in cols:
        if name == "utf8":
            dev.append(ctx.upload(vals, valid))
        elif name in tt.TEMPORAL:
            dev.append(ctx.upload_arrow(temporal(vals, valid, typ, phys)))
        else:
            dev.append(ctx.upload(np.asarray(vals, np.int64), valid))
    return dev


def host_pg(cols):
    return [(name, [None if (valid is not None and not valid[i]) else (vals[i] if name == "utf8" else int(vals[i]))
                    for i in range(len(vals))]) for name, vals, valid, _, _ in cols]


@pytest.mark.gpu
@pytest.mark.parametrize("n,shape", [(1, "wide"), (255, "wide"), (256, "wide"), (257, "wide"), (3000, "wide"),
                                     (3000, "narrow"), (3000, "long")])
def test_pg_datarows_temporal_text(ctx, n, shape):
    """Byte for byte against tests/temporal_text.py framed by oracle/pg_text.py: one workgroup stages 256
    rows, so the row counts cover one row, the boundary, a partial tile and several tiles; the three
    shapes take the 16 KB stage, the 48 KB stage and the direct write."""
    cols = pg_columns(n, shape, seed=n + len(shape))
    want = tt.encode_rows(host_pg(cols))
    total = sum(len(w) for w in want)
    if n == 3000:  # the shapes do select the three write paths (k_encode.hip: total <= 56 n -> 16 KB stage)
        tile = max(sum(len(w) for w in want[i:i + 256]) for i in range(0, n, 256))
        assert {"narrow": total <= 56 * n and tile <= 16384, "wide": total > 56 * n and tile <= 49152,
                "long": tile > 49152}[shape]
    got = ctx.encode_pg_datarows(upload_pg(ctx, cols)).to_bytes()
    assert len(got) == len(want) == n
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (i, g, w)
    if shape == "wide":  # the column order and a NULL's field length -1
        assert got[0][5:7] == (8).to_bytes(2, "big") and got[0][7:21] == b"\x00\x00\x00\x0a1970-01-01"
        nulls = [i for i in range(n) if not cols[0][2][i]]
        assert all(got[i][7:11] == b"\xff\xff\xff\xff" for i in nulls)


@pytest.mark.gpu
@pytest.mark.parametrize("name,bad", [("date32", DAY_MAX + 1), ("date32", DAY_MIN - 1), ("date64", (DAY_MAX + 1) * 86400000),
                                      ("ts_s", (DAY_MAX + 1) * 86400), ("ts_us", (DAY_MIN * 86400 - 1) * 10 ** 6)])
def test_pg_datarows_year_outside_the_range_is_refused(ctx, name, bad):
    _, typ, _, phys = next(t for t in TYPES if t[0] == name)
    n = 3000
    vals = np.zeros(n, np.int64)
    vals[1234] = bad
    i64 = ctx.upload(np.arange(n, dtype=np.int64))
    with pytest.raises(QehError) as e:
        ctx.encode_pg_datarows([i64, ctx.upload_arrow(temporal(vals, None, typ, phys))])
    assert e.value.status == abi.QEH_E_UNSUPPORTED and "year outside 0000-9999" in e.value.message
    # the same value in a NULL row is never looked at
    valid = np.ones(n, bool)
    valid[1234] = False
    got = ctx.encode_pg_datarows([i64, ctx.upload_arrow(temporal(vals, valid, typ, phys))]).to_bytes()
    want = tt.encode_rows([("int64", list(range(n))), (name, [None if i == 1234 else 0 for i in range(n)])])
    assert got == want
