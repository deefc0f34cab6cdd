"""Utf8 GROUP BY / ORDER BY / window keys on the device.

qeh_utf8_dict_encode turns a Utf8 column into INT32 codes whose integer order is the strings'
byte-wise (unsigned) lexicographic order, and the sort, aggregate and window entry points group and
order Utf8 keys through those codes.

Expected values never come from the code under test: Python `bytes` compare in unsigned
lexicographic order (arrow's order on StringArray), so the expected dictionary is
sorted(set(non-NULL rows)), the expected codes are a dict lookup, and sort / window / group-by are
the CPU oracle's over those Python-computed codes as Int32 keys with the same validity (exact
equality; group-by compared as a mapping)."""
import os
import re

import numpy as np
import pyarrow as pa
import pyarrow.csv as pacsv
import pytest

import oracle_bind as ob
import qe_hip
from qe_hip import AggregateExpr, AggregateFunction as AF, BinaryOp, abi, binop, col, lit
from qe_hip import HashAggregate, HashJoin, JoinType, MemoryDataSource, QueryExecutor, Scan, Sort, WindowFunctionType
from qe_hip.device import unpack_bits
from qe_hip.expr import Column

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

PREFIX40 = b"0123456789abcdefghij0123456789ABCDEFGHIJ"
# the contents at which an order-preserving encoding can go wrong
POOL = [
    b"", None,                                             # the empty string is a value, not NULL
    b"a", b"a\x00", b"a\x00\x00", b"ab",                   # a longer string that only adds 0x00 bytes
    b"1234567", b"12345678", b"123456789",                 # lengths around one 8-byte word
    b"123456789012345", b"1234567890123456", b"12345678901234567",  # ... and around two
    b"\x7f", b"\x80", b"\xff", b"z\x80", b"z\x7f", b"\xc3\xa9t\xc3\xa9", b"ete",  # a signed compare misorders these
    PREFIX40, PREFIX40 + b"a", PREFIX40 + b"b", PREFIX40 + b"\x80", PREFIX40 + b"\x00",  # six rounds to tell apart
    b"1234567\x00", b"12345678\x00", b"Engineering", b"Sales", b"HR",
    b"Marketing", b"Building A", b"Building B", b"Building", b"zz", b"Z", b"0", b" ", b"\x00",
]
assert len(PREFIX40) == 40 and len(set(POOL)) == len(POOL) == 38  # 37 distinct strings and NULL


# ---- CPU: the boundary ------------------------------------------------------------------------

def test_prototype_is_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "qeh.h")).read()
    assert "#define QEH_ABI_VERSION 1" in src  # additive change
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"^\s*int\s+qeh_utf8_dict_encode\s*\(([^)]*)\)\s*;", code, flags=re.M)
    assert m, "qeh_utf8_dict_encode is not declared in include/qeh.h"
    assert m.group(1).count("qeh_column") == 3 and "qeh_ctx" in m.group(1)
    assert "qeh_utf8_dict_encode" in abi.SIGNATURES
    restype, argtypes = abi.SIGNATURES["qeh_utf8_dict_encode"]
    assert len(argtypes) == 4
    assert hasattr(qe_hip.load(), "qeh_utf8_dict_encode")
    assert hasattr(qe_hip.Context, "utf8_dict_encode")


# ---- helpers ------------------------------------------------------------------------------------

def py_encode(strs):
    """(expected dictionary, Int32 codes with 0 at NULL rows, validity) computed in Python."""
    dic = sorted({s for s in strs if s is not None})
    code = {s: i for i, s in enumerate(dic)}
    codes = np.array([0 if s is None else code[s] for s in strs], np.int32)
    valid = np.array([s is not None for s in strs], bool)
    return dic, codes, valid


def host_key(strs):
    """The Python-computed codes as an oracle key column."""
    _, codes, valid = py_encode(strs)
    return ob.HostCol(codes, None if valid.all() else valid)


def utf8_rows(c):
    """Device Utf8 column -> list of bytes / None."""
    vals = c.to_bytes()
    n, off = c.c.length, c.c.offset
    if c.c.validity and n:
        vb = np.empty((off + n + 7) // 8, np.uint8)
        c.ctx.d2h(vb, c.c.validity, len(vb))
        valid = unpack_bits(vb, n, off)
        return [v if ok else None for v, ok in zip(vals, valid)]
    return vals


def check_encode(ctx, strs, column=None):
    column = ctx.upload(list(strs)) if column is None else column
    codes, dic = ctx.utf8_dict_encode(column)
    want_dic, want_codes, want_valid = py_encode(strs)
    assert dic.dtype == abi.DT_UTF8 and len(dic) == len(want_dic)
    assert not dic.c.validity, "the dictionary carries no NULLs"
    assert dic.to_bytes() == want_dic
    assert codes.dtype == abi.DT_INT32 and len(codes) == len(strs)
    got_codes, got_valid = codes.to_numpy()
    assert got_codes.dtype == np.int32
    assert np.array_equal(got_codes, want_codes)
    if want_valid.all():
        assert got_valid is None or got_valid.all()
    else:
        assert got_valid is not None and np.array_equal(got_valid, want_valid)


def pooled(n, seed):
    r = np.random.default_rng(seed)
    return [POOL[i] for i in r.integers(0, len(POOL), n)]


# ---- encode -------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 4097])
def test_encode_sizes(ctx, n):
    strs = pooled(n, 100 + n)
    if n >= 63:
        strs[:len(POOL)] = POOL  # every special value is present
    check_encode(ctx, strs)


@pytest.mark.gpu
def test_encode_all_null_all_equal_and_no_nulls(ctx):
    check_encode(ctx, [None] * 65)
    check_encode(ctx, [b"same string, longer than a word"] * 130)
    check_encode(ctx, [b""] * 3)
    check_encode(ctx, [s for s in pooled(300, 7) if s is not None])


@pytest.mark.gpu
def test_encode_honours_offset(ctx):
    strs = pooled(200, 11)
    strs[0] = b"bytes before the slice"  # the slice's first offset is not 0
    base = ctx.upload(list(strs))
    sl = ctx.slice(base, 37, 101)
    assert sl.c.offset == 37
    check_encode(ctx, strs[37:138], sl)


@pytest.mark.gpu
def test_encode_many_workgroups_few_strings(ctx):
    """70 001 rows over 300 distinct strings: several workgroups race for the same slots."""
    pool = [b"key-%03d-" % i + bytes([i % 256]) * (i % 19) for i in range(300)]
    r = np.random.default_rng(5)
    strs = [pool[i] for i in r.integers(0, 300, 70_001)]
    check_encode(ctx, strs)


def distinct5000():
    r = np.random.default_rng(9)
    strs = [b"s%05d" % i + b"\x80\x00tail"[: i % 7] for i in range(5000)]
    return [strs[i] for i in r.permutation(5000)]


@pytest.mark.gpu
@pytest.mark.parametrize("seam", [None, ("QEH_UTF8_DICT_CAP_LOG2", "4"), ("QEH_UTF8_DICT_HASH_BITS", "3")])
def test_encode_all_distinct_growth_and_hash_collisions(ctx, monkeypatch, seam):
    """5 000 distinct strings; again from a 16-slot table (growth) and with the hash masked to 3 bits
    (equal hash and tag, different bytes: compare, then probe on).  Same result each time."""
    if seam:
        monkeypatch.setenv(*seam)
    ctx.timing(True)
    ctx.timing_reset()
    try:
        check_encode(ctx, distinct5000())
        launches = ctx.kernel_time("utf8_dict_insert")[1]
    finally:
        ctx.timing(False)
    # the default table (2^14 slots) holds 5 000 strings in one pass; from 16 slots it grows
    # 16 -> 256 -> 2^14, so the seam is seen to act
    assert launches == (3 if seam and seam[0] == "QEH_UTF8_DICT_CAP_LOG2" else 1)


# ---- sort ---------------------------------------------------------------------------------------

N = 4097


@pytest.fixture(scope="module")
def keyed():
    """4097 rows: a Utf8 key of ~30 distinct strings with NULLs, an Int64 key, an Int64 value."""
    r = np.random.default_rng(21)
    strs = pooled(N, 22)
    ik = r.integers(-3, 4, N).astype(np.int64)
    v = r.integers(-(2 ** 40), 2 ** 40, N).astype(np.int64)
    return strs, ik, v


@pytest.mark.gpu
@pytest.mark.parametrize("asc", [True, False])
def test_sort_one_utf8_key(ctx, keyed, asc):
    strs = keyed[0]
    got = ctx.sort_indices([ctx.upload(list(strs))], [asc]).to_numpy()[0]
    want = ob.sort_indices([host_key(strs)], [asc])
    assert np.array_equal(got, want)  # duplicates keep input order (stable)


@pytest.mark.gpu
def test_sort_nulls_last(ctx, keyed):
    strs = keyed[0]
    got = ctx.sort_indices_nulls([ctx.upload(list(strs))], [True], [False]).to_numpy()[0]
    want = ob.sort_indices_nulls([host_key(strs)], [True], [False])
    assert np.array_equal(got, want)
    assert strs[int(got[-1])] is None


@pytest.mark.gpu
@pytest.mark.parametrize("utf8_first", [True, False])
def test_sort_two_keys(ctx, keyed, utf8_first):
    strs, ik, _ = keyed
    dev = [ctx.upload(list(strs)), ctx.upload(ik)]
    host = [host_key(strs), ob.HostCol(ik)]
    if not utf8_first:
        dev, host = dev[::-1], host[::-1]
    got = ctx.sort_indices(dev, [True, False]).to_numpy()[0]
    assert np.array_equal(got, ob.sort_indices(host, [True, False]))


# ---- group-by -----------------------------------------------------------------------------------

AGGS = [(AF.Count, 0), (AF.Sum, 0), (AF.Min, 0), (AF.Max, 0), (AF.Avg, 0)]


def mapping(key_cols, agg_cols, n):
    """{key tuple: aggregate tuple}; key_cols are lists (None = NULL), agg_cols (values, valid)."""
    out = {}
    for g in range(n):
        k = tuple(kc[g] for kc in key_cols)
        a = tuple((vals[g].item(), True) if valid is None or valid[g] else (None, False) for vals, valid in agg_cols)
        assert k not in out, f"group {k!r} appears twice"
        out[k] = a
    return out


def int_rows(vals, valid):
    return [v.item() if valid is None or valid[i] else None for i, v in enumerate(vals)]


def oracle_groups(key_specs, inputs, aggs):
    """key_specs: ('utf8', strs) or ('int', values).  The oracle groups on the Python codes; the
    codes are mapped back through the Python dictionary."""
    hk = [host_key(x) if kind == "utf8" else ob.HostCol(x) for kind, x in key_specs]
    wk, wa, g, _ = ob.hash_aggregate(hk, inputs, aggs)
    keys = []
    for (kind, x), (vals, valid) in zip(key_specs, wk):
        rows = int_rows(vals, valid)
        if kind == "utf8":
            dic = py_encode(x)[0]
            rows = [None if c is None else dic[c] for c in rows]
        keys.append(rows)
    return mapping(keys, wa, g)


def device_groups(key_specs, gk, ga, g):
    keys = [utf8_rows(c) if kind == "utf8" else int_rows(*c.to_numpy()) for (kind, _), c in zip(key_specs, gk)]
    for (kind, _), c in zip(key_specs, gk):
        assert c.dtype == (abi.DT_UTF8 if kind == "utf8" else abi.DT_INT64)
    return mapping(keys, [c.to_numpy() for c in ga], g)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["utf8", "utf8_int", "utf8_utf8"])
def test_hash_aggregate_utf8_keys(ctx, keyed, shape):
    strs, ik, v = keyed
    other = [POOL[(i * 5) % 7 + 2] for i in range(N)]
    specs = {"utf8": [("utf8", strs)], "utf8_int": [("utf8", strs), ("int", ik)],
             "utf8_utf8": [("utf8", strs), ("utf8", other)]}[shape]
    dev_keys = [ctx.upload(list(x)) if kind == "utf8" else ctx.upload(x) for kind, x in specs]
    gk, ga, g = ctx.hash_aggregate(dev_keys, [ctx.upload(v)], AGGS)
    got = device_groups(specs, gk, ga, g)
    want = oracle_groups(specs, [ob.HostCol(v)], AGGS)
    if shape == "utf8":
        assert None in [k[0] for k in want], "the NULL group is part of the case"
        assert (b"",) in want
    assert got == want


@pytest.mark.gpu
def test_hash_aggregate_every_row_distinct(ctx):
    strs = distinct5000()[:N]
    v = np.arange(N, dtype=np.int64) * 3 - 5000
    gk, ga, g = ctx.hash_aggregate([ctx.upload(list(strs))], [ctx.upload(v)], AGGS)
    assert g == N
    assert device_groups([("utf8", strs)], gk, ga, g) == oracle_groups([("utf8", strs)], [ob.HostCol(v)], AGGS)


@pytest.mark.gpu
def test_filter_aggregate_drops_one_string(ctx, keyed):
    strs, _, v = keyed
    gone = b"Engineering"
    flag = np.array([1 if s == gone else 0 for s in strs], np.int64)
    assert flag.sum() > 0
    pred = binop(col(2), BinaryOp.Equal, lit(0))
    aggs = [(f, 1) for f, _ in AGGS]
    gk, ga, g = ctx.filter_aggregate([ctx.upload(list(strs)), ctx.upload(v), ctx.upload(flag)], pred, [0], aggs)
    got = device_groups([("utf8", strs)], gk, ga, g)
    kept = [i for i in range(N) if flag[i] == 0]
    want = oracle_groups([("utf8", [strs[i] for i in kept])], [ob.HostCol(v[kept]), ob.HostCol(v[kept])], aggs)
    assert (gone,) not in got and (None,) in got
    assert got == want


# ---- window -------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_row_number_partition_by_utf8(ctx, keyed):
    strs, _, v = keyed
    got = ctx.row_number([ctx.upload(list(strs))], [ctx.upload(v)], [True]).to_numpy()[0]
    want = ob.row_number([host_key(strs)], [ob.HostCol(v)], [True])
    assert np.array_equal(got, want)


@pytest.mark.gpu
def test_rank_order_by_utf8_descending(ctx, keyed):
    strs, ik, _ = keyed
    got = ctx.window(WindowFunctionType.Rank, [ctx.upload(ik)], [ctx.upload(list(strs))], [False]).to_numpy()[0]
    want, _ = ob.window(WindowFunctionType.Rank, [ob.HostCol(ik)], [host_key(strs)], [False])
    assert np.array_equal(got, want)


# ---- what stays off the device ------------------------------------------------------------------

@pytest.mark.gpu
def test_out_of_scope_utf8_uses_are_refused(ctx):
    """Utf8 join, merge and range-partition keys and a Utf8 LAG argument are
    QEH_E_UNSUPPORTED; MIN of a Utf8 column is the reference's type error."""
    strs = [b"b", b"a", None, b"c"]
    s, s2 = ctx.upload(list(strs)), ctx.upload([b"a", b"c", b"d", b"e"])
    v = ctx.upload(np.arange(4, dtype=np.int64))

    def status_of(fn):
        with pytest.raises(qe_hip.QehError) as e:
            fn()
        return e.value.status

    assert status_of(lambda: ctx.hash_join_inner(s, [v], s2, [v])) == abi.QEH_E_UNSUPPORTED
    assert status_of(lambda: ctx.merge_sorted([[s, v, v], [s2, v, v]], [0], [True], [True])) == abi.QEH_E_UNSUPPORTED
    assert status_of(lambda: ctx.range_partition(s, [1], True)) == abi.QEH_E_UNSUPPORTED
    assert status_of(lambda: ctx.window(WindowFunctionType.Lag, [v], [v], [True], arg=s, param=1)) == abi.QEH_E_UNSUPPORTED
    assert status_of(lambda: ctx.hash_aggregate([v], [s], [(AF.Min, 0)])) == abi.QEH_E_TYPE
    assert status_of(lambda: ctx.hash_aggregate([s], [s], [(AF.Max, 0)])) == abi.QEH_E_TYPE  # before any encode


# ---- plan level ---------------------------------------------------------------------------------

def sources():
    emp = pacsv.read_csv(os.path.join(GOLD, "employees.csv"))  # "NULL" is read as a NULL
    dep = pacsv.read_csv(os.path.join(GOLD, "departments.csv"))
    e2 = emp.rename_columns([f"employees.{c}" for c in emp.column_names])
    d2 = dep.rename_columns([f"departments.{c}" for c in dep.column_names])
    return emp, dep, MemoryDataSource(e2.schema, e2.to_batches()), MemoryDataSource(d2.schema, d2.to_batches())


@pytest.mark.gpu
def test_plan_order_by_name_descending(ctx):
    emp, _, es, _ = sources()
    out = QueryExecutor(ctx).execute(Sort(Scan(es), [Column("employees.name", 1)], [False]))
    t = pa.Table.from_batches(out)
    rows = list(zip(*[emp.column(i).to_pylist() for i in range(emp.num_columns)]))
    want = sorted(rows, key=lambda r: r[1].encode(), reverse=True)  # names are distinct and non-NULL
    assert len({r[1] for r in rows}) == len(rows)
    assert list(zip(*[t.column(i).to_pylist() for i in range(t.num_columns)])) == want


@pytest.mark.gpu
def test_plan_group_by_dept_name_over_join(ctx):
    """SELECT dept_name, COUNT(*), AVG(salary) FROM employees JOIN departments USING (dept_id)
    GROUP BY dept_name."""
    emp, dep, es, ds = sources()
    on = binop(Column("employees.dept_id", 4), BinaryOp.Equal, Column("departments.dept_id", 5))
    plan = HashAggregate(HashJoin(Scan(es), Scan(ds), JoinType.Inner, on), [Column("departments.dept_name", 6)],
                         [AggregateExpr(AF.Count, Column("employees.id", 0)),
                          AggregateExpr(AF.Avg, Column("employees.salary", 3))])
    t = pa.Table.from_batches(QueryExecutor(ctx).execute(plan))
    assert t.schema.field(0).type == pa.string()
    got = {k: (c, a) for k, c, a in zip(*[t.column(i).to_pylist() for i in range(3)])}
    names = dict(zip(dep["dept_id"].to_pylist(), dep["dept_name"].to_pylist()))
    sal = {}
    for d, s in zip(emp["dept_id"].to_pylist(), emp["salary"].to_pylist()):
        if d is not None and d in names:  # a NULL dept_id matches nothing
            sal.setdefault(names[d], []).append(s)
    want = {k: (len(v), float(sum(v)) / len(v)) for k, v in sal.items()}
    assert len(want) >= 2
    assert got == want
