"""Utf8 equi-join keys through a shared device dictionary.

qeh_utf8_join_encode gives two Utf8 columns INT32 codes from one dictionary built over the build
column (equal codes <=> equal bytes, dense in [0, D), unordered; a probe string the build side
lacks is NULL), qeh_hash_join joins on those codes, and the plan executor keys HashJoin -- alone,
under a fused aggregate and in a multi-conjunct `on` -- on them.

Expected values never come from the code under test: a join's expected rows are computed in Python
(a dict from key bytes to row lists gives multisets of row tuples, None for the NULL side), and code
columns are checked as a mapping, not as particular numbers."""
import os
import re
from collections import Counter

import numpy as np
import pyarrow as pa
import pyarrow.csv as pacsv
import pytest

import qe_hip
from qe_hip import AggregateExpr, AggregateFunction as AF, BinaryOp, abi, binop, lit
from qe_hip import Filter, HashAggregate, HashJoin, JoinType, MemoryDataSource, QueryExecutor, Scan
from qe_hip.device import unpack_bits
from qe_hip.expr import Column

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

PREFIX40 = b"0123456789abcdefghij0123456789ABCDEFGHIJ"
# the contents at which a hashed, byte-compared dictionary can go wrong
POOL = [
    b"",                                                   # the empty string is a value, not NULL
    b"a", b"a\x00", b"a\x00\x00", b"ab",                   # a longer string that only adds 0x00 bytes
    b"1234567", b"12345678", b"123456789",                 # lengths around one 8-byte word
    b"123456789012345", b"1234567890123456", b"12345678901234567",  # ... and around two
    b"\x7f", b"\x80", b"\xff", b"z\x80", b"z\x7f", b"\xc3\xa9t\xc3\xa9", b"ete",  # bytes around 0x80
    PREFIX40, PREFIX40 + b"a", PREFIX40 + b"b", PREFIX40 + b"\x80", PREFIX40 + b"\x00",  # long shared prefix
    b"1234567\x00", b"12345678\x00", b"Engineering", b"Sales", b"HR", b"Marketing", b"\x00", b" ",
] + [b"key-%04d" % i + bytes([i % 251]) * (i % 23) for i in range(600)]
assert len(set(POOL)) == len(POOL)


# ---- CPU: the boundary ------------------------------------------------------------------------

def test_prototypes_are_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "qeh.h")).read()
    assert "#define QEH_ABI_VERSION 1" in src  # additive change
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, n_cols, n_args, method in [("qeh_utf8_join_encode", 4, 6, "utf8_join_encode"),
                                         ("qeh_hash_join", 6, 11, "hash_join")]:
        m = re.search(r"^\s*int\s+%s\s*\(([^)]*)\)\s*;" % name, code, flags=re.M)
        assert m, f"{name} is not declared in include/qeh.h"
        assert m.group(1).count("qeh_column") == n_cols and "qeh_ctx" in m.group(1)
        assert name in abi.SIGNATURES
        assert len(abi.SIGNATURES[name][1]) == n_args
        assert hasattr(qe_hip.load(), name), f"libqeh.so does not export {name}"
        assert hasattr(qe_hip.Context, method)


# ---- helpers ------------------------------------------------------------------------------------

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


def col_rows(c):
    """Device column -> list of Python values, None = NULL."""
    if c.dtype == abi.DT_UTF8:
        return utf8_rows(c)
    vals, valid = c.to_numpy()
    return [v.item() if valid is None or valid[i] else None for i, v in enumerate(vals)]


def py_join(jt, lkeys, lrows, rkeys, rrows):
    """Multiset of (left row ++ right row) tuples of the equi-join; a NULL key matches nothing."""
    wl = len(lrows[0]) if lrows else 0
    wr = len(rrows[0]) if rrows else 0
    by_key = {}
    for j, k in enumerate(rkeys):
        if k is not None:
            by_key.setdefault(k, []).append(j)
    out, hit = Counter(), set()
    for i, k in enumerate(lkeys):
        js = by_key.get(k, []) if k is not None else []
        for j in js:
            out[tuple(lrows[i]) + tuple(rrows[j])] += 1
            hit.add(j)
        if not js and jt in (JoinType.Left, JoinType.Full):
            out[tuple(lrows[i]) + (None,) * wr] += 1
    if jt in (JoinType.Right, JoinType.Full):
        for j in range(len(rkeys)):
            if j not in hit:
                out[(None,) * wl + tuple(rrows[j])] += 1
    return out


def check_join_encode(ctx, build, probe, build_col=None, probe_col=None):
    bcol = ctx.upload(list(build)) if build_col is None else build_col
    pcol = ctx.upload(list(probe)) if probe_col is None else probe_col
    bc, pc, d = ctx.utf8_join_encode(bcol, pcol)
    assert bc.dtype == abi.DT_INT32 and pc.dtype == abi.DT_INT32
    assert len(bc) == len(build) and len(pc) == len(probe)
    bset = {s for s in build if s is not None}
    assert d == len(bset)
    bcodes, bvalid = bc.to_numpy()
    if bvalid is None:
        bvalid = np.ones(len(build), bool)
    assert np.array_equal(bvalid, np.array([s is not None for s in build], bool))
    code_of = {}
    for s, c, v in zip(build, bcodes.tolist(), bvalid):
        if v:
            assert 0 <= c < d
            assert code_of.setdefault(s, c) == c, "string -> code is not a function"
    assert len(set(code_of.values())) == len(code_of) == d, "string -> code is not injective"
    assert pc.c.validity or len(probe) == 0, "probe codes carry a validity bitmap"
    pcodes, pvalid = pc.to_numpy()
    if len(probe) == 0:
        return
    assert np.array_equal(pvalid, np.array([s is not None and s in bset for s in probe], bool))
    want = np.array([code_of.get(s, 0) if s is not None else 0 for s in probe], np.int32)
    assert np.array_equal(pcodes, want)  # invalid rows hold 0


def encode_inputs():
    r = np.random.default_rng(31)
    build_pool = POOL[:31] + POOL[31:431]        # every special string and 400 plain ones
    absent = POOL[431:]                          # 200 strings the build side lacks
    build = [build_pool[i] for i in r.integers(0, len(build_pool), 5000)]
    build[:31] = POOL[:31]
    for i in r.integers(31, 5000, 250):
        build[i] = None
    probe_pool = build_pool + absent + [None] * 40 + [b""] * 10 + [PREFIX40 + b"c", b"a\x00\x00\x00", b"12345678\x00\x00"]
    probe = [probe_pool[i] for i in r.integers(0, len(probe_pool), 8191)]
    return build, probe


# ---- encode -------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("seam", [None, ("QEH_UTF8_DICT_CAP_LOG2", "4"), ("QEH_UTF8_DICT_HASH_BITS", "3")])
def test_join_encode_contract(ctx, monkeypatch, seam):
    """Default; from a 16-slot table (growth before the lookup); with the hash masked to 3 bits
    (strings share hash and tag but differ in bytes: the lookup compares bytes and probes on, and an
    absent string that shares a tag comes out absent).  Same result each time."""
    if seam:
        monkeypatch.setenv(*seam)
    build, probe = encode_inputs()
    assert None in build and None in probe and b"" in build and b"" in probe
    assert any(s is not None and s not in set(build) for s in probe)
    ctx.timing(True)
    ctx.timing_reset()
    try:
        check_join_encode(ctx, build, probe)
        inserts, lookups = ctx.kernel_time("utf8_dict_insert")[1], ctx.kernel_time("utf8_dict_lookup")[1]
        orders = ctx.kernel_time("utf8_dict_order")[1]
    finally:
        ctx.timing(False)
    assert lookups == 1 and orders == 0  # one streaming pass; no ordering rounds on this path
    assert inserts == (3 if seam and seam[0] == "QEH_UTF8_DICT_CAP_LOG2" else 1)  # the seam is seen to act


@pytest.mark.gpu
def test_join_encode_edges(ctx):
    some = [b"x", None, b"", b"yy", b"x"]
    check_join_encode(ctx, [], some)                      # empty build side: D = 0, nothing matches
    check_join_encode(ctx, some, [])                      # empty probe side
    check_join_encode(ctx, [], [])
    check_join_encode(ctx, [None] * 65, some * 13)        # all-NULL build side
    check_join_encode(ctx, [b"z"] + [b"only once, and longer than two words"] + [b"q"] * 3,
                      [b"only once, and longer than two words"] * 4096)
    check_join_encode(ctx, [s for s in some if s is not None], [b"x", b"yy", b""])  # no bitmap on either input


@pytest.mark.gpu
def test_join_encode_honours_offsets(ctx):
    build, probe = encode_inputs()
    build, probe = build[:300], probe[:400]
    build[0] = probe[0] = b"bytes before the slice"       # the slices' first offsets are not 0
    bs, ps = ctx.slice(ctx.upload(list(build)), 37, 201), ctx.slice(ctx.upload(list(probe)), 65, 300)
    assert bs.c.offset == 37 and ps.c.offset == 65
    check_join_encode(ctx, build[37:238], probe[65:365], bs, ps)


# ---- qeh_hash_join ------------------------------------------------------------------------------

NL, NR = 4097, 1031


@pytest.fixture(scope="module")
def sides():
    """4097 x 1031 rows: duplicate keys and NULL keys on both sides, strings absent in both
    directions; per side an Int64 payload and the Utf8 key itself as a payload."""
    r = np.random.default_rng(41)
    lpool, rpool = POOL[:450] + [None] * 20, POOL[200:631] + [None] * 20
    lk = [lpool[i] for i in r.integers(0, len(lpool), NL)]
    rk = [rpool[i] for i in r.integers(0, len(rpool), NR)]
    lk[:31] = POOL[:31]
    rk[:31] = POOL[:31]
    lid = np.arange(NL, dtype=np.int64) * 7 - 1000
    rid = np.arange(NR, dtype=np.int64) * 3 + (1 << 40)
    return lk, lid, rk, rid


@pytest.mark.gpu
@pytest.mark.parametrize("jt", [JoinType.Inner, JoinType.Left, JoinType.Right, JoinType.Full])
def test_hash_join_utf8_keys(ctx, sides, jt):
    lk, lid, rk, rid = sides
    dl, dr = ctx.upload(list(lk)), ctx.upload(list(rk))
    ol, orr, rows = ctx.hash_join(jt, dl, [ctx.upload(lid), dl], dr, [ctx.upload(rid), dr])
    assert [c.dtype for c in ol + orr] == [abi.DT_INT64, abi.DT_UTF8, abi.DT_INT64, abi.DT_UTF8]
    cols = [col_rows(c) for c in ol + orr]
    assert all(len(c) == rows for c in cols)
    got = Counter(zip(*cols))
    want = py_join(jt, lk, list(zip(lid.tolist(), lk)), rk, list(zip(rid.tolist(), rk)))
    assert sum(want.values()) > max(NL, NR)  # duplicates on both sides multiply
    assert got == want  # the Utf8 key columns come back as the original strings


@pytest.mark.gpu
def test_hash_join_forwards_integer_keys_and_refuses_mixed(ctx, sides):
    lk, lid, rk, rid = sides
    a, b = ctx.upload(lid % 50), ctx.upload(rid % 50)
    ol, orr, rows = ctx.hash_join(JoinType.Left, a, [a], b, [b])
    want = py_join(JoinType.Left, (lid % 50).tolist(), [(x,) for x in (lid % 50).tolist()],
                   (rid % 50).tolist(), [(x,) for x in (rid % 50).tolist()])
    assert Counter(zip(col_rows(ol[0]), col_rows(orr[0]))) == want
    for args in [(ctx.upload(list(lk)), [a], ctx.upload(np.arange(NL, dtype=np.int64)), [a]),
                 (a, [a], ctx.upload(list(lk)), [a])]:
        with pytest.raises(qe_hip.QehError) as e:
            ctx.hash_join(JoinType.Inner, *args)
        assert e.value.status == abi.QEH_E_TYPE
    with pytest.raises(qe_hip.QehError, match="Invalid argument error: Invalid comparison operation: Utf8 == Int64"):
        ctx.hash_join(JoinType.Inner, ctx.upload(list(lk)), [a], ctx.upload(np.arange(NL, dtype=np.int64)), [a])


# ---- plan level ---------------------------------------------------------------------------------

def table_rows(t):
    cols = [[v.encode() if isinstance(v, str) else v for v in t.column(i).to_pylist()] for i in range(t.num_columns)]
    return list(zip(*cols)) if t.num_rows else []


def source(t, prefix):
    t2 = t.rename_columns([f"{prefix}.{c}" for c in t.column_names])
    return MemoryDataSource(t2.schema, t2.to_batches())


def golden_sources():
    """The golden employees with a dept_name column: mapped from dept_id, None where there is no
    department, and one name no department has."""
    emp = pacsv.read_csv(os.path.join(GOLD, "employees.csv"))  # "NULL" is read as a NULL
    dep = pacsv.read_csv(os.path.join(GOLD, "departments.csv"))
    names = dict(zip(dep["dept_id"].to_pylist(), dep["dept_name"].to_pylist()))
    dn = [names.get(d) for d in emp["dept_id"].to_pylist()]
    assert None in dn
    dn[4] = "Research"
    assert set(names.values()) - set(dn), "a department without employees is part of the case"
    emp = emp.append_column("dept_name", pa.array(dn, pa.string()))
    return emp, dep


def run_plan(ctx, plan):
    ctx.timing(True)
    ctx.timing_reset()
    try:
        t = pa.Table.from_batches(QueryExecutor(ctx).execute(plan))
        lookups = ctx.kernel_time("utf8_dict_lookup")[1]
    finally:
        ctx.timing(False)
    return t, lookups


E_DEPT_NAME, D_DEPT_NAME, D_LOCATION = 5, 7, 8  # employees has 6 columns, then departments' 4


@pytest.mark.gpu
@pytest.mark.parametrize("jt", [JoinType.Inner, JoinType.Left, JoinType.Right, JoinType.Full])
def test_plan_hash_join_on_string_key(ctx, jt):
    emp, dep = golden_sources()
    on = binop(Column("employees.dept_name", E_DEPT_NAME), BinaryOp.Equal, Column("departments.dept_name", D_DEPT_NAME))
    t, lookups = run_plan(ctx, HashJoin(Scan(source(emp, "employees")), Scan(source(dep, "departments")), jt, on))
    er, dr = table_rows(emp), table_rows(dep)
    want = py_join(jt, [r[5] for r in er], er, [r[1] for r in dr], dr)
    assert t.num_columns == 10 and t.schema.field(E_DEPT_NAME).type == pa.string()
    assert Counter(table_rows(t)) == want
    assert lookups >= 1, "the join did not key on the shared dictionary codes"


@pytest.mark.gpu
@pytest.mark.parametrize("filtered,no_fusion", [(True, False), (False, False), (True, True), (False, True)])
def test_plan_aggregate_over_string_key_join(ctx, monkeypatch, filtered, no_fusion):
    """SELECT d.location, COUNT(e.id), SUM(e.salary), COUNT(e.dept_name) FROM e JOIN d
    ON e.dept_name = d.dept_name [WHERE e.salary > 76000] GROUP BY d.location."""
    if no_fusion:
        monkeypatch.setenv("QEH_NO_FUSION", "1")
    emp, dep = golden_sources()
    on = binop(Column("employees.dept_name", E_DEPT_NAME), BinaryOp.Equal, Column("departments.dept_name", D_DEPT_NAME))
    node = HashJoin(Scan(source(emp, "employees")), Scan(source(dep, "departments")), JoinType.Inner, on)
    if filtered:
        node = Filter(node, binop(Column("employees.salary", 3), BinaryOp.Greater, lit(76000)))
    plan = HashAggregate(node, [Column("departments.location", D_LOCATION)],
                         [AggregateExpr(AF.Count, Column("employees.id", 0)),
                          AggregateExpr(AF.Sum, Column("employees.salary", 3)),
                          AggregateExpr(AF.Count, Column("employees.dept_name", E_DEPT_NAME))])
    t, lookups = run_plan(ctx, plan)
    er, dr = table_rows(emp), table_rows(dep)
    want = {}
    for row, k in py_join(JoinType.Inner, [r[5] for r in er], er, [r[1] for r in dr], dr).items():
        if filtered and not row[3] > 76000:
            continue
        c, s, cn = want.get(row[D_LOCATION], (0, 0, 0))
        want[row[D_LOCATION]] = (c + k, s + k * row[3], cn + k * (row[E_DEPT_NAME] is not None))
    assert len(want) >= 2
    got = {r[0]: r[1:] for r in table_rows(t)}
    assert len(got) == t.num_rows and got == want
    assert lookups >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("jt", [JoinType.Inner, JoinType.Full])
def test_plan_join_past_the_cartesian_limit(ctx, jt):
    """70 000 x 70 000 rows (a product beyond 2^32), 35 000 strings shared."""
    n, shift = 70_000, 35_000
    lt = pa.table({"id": pa.array(np.arange(n, dtype=np.int64)),
                   "s": pa.array(["k%07d" % i for i in range(n)], pa.string())})
    rt = pa.table({"id": pa.array(np.arange(shift, shift + n, dtype=np.int64)),
                   "s": pa.array(["k%07d" % i for i in range(shift, shift + n)], pa.string())})
    on = binop(Column("l.s", 1), BinaryOp.Equal, Column("r.s", 3))
    t, lookups = run_plan(ctx, HashJoin(Scan(source(lt, "l")), Scan(source(rt, "r")), jt, on))
    assert t.num_rows == (n - shift if jt == JoinType.Inner else 2 * n - (n - shift))
    lid, ls = np.array(t.column(0).to_pylist(), object), t.column(1).to_pylist()
    rid, rs = np.array(t.column(2).to_pylist(), object), t.column(3).to_pylist()
    both = np.array([a is not None and b is not None for a, b in zip(lid, rid)], bool)
    assert both.sum() == n - shift
    assert all(lid[i] == rid[i] and ls[i] == rs[i] == "k%07d" % lid[i] for i in np.flatnonzero(both))
    assert sorted(lid[both]) == list(range(shift, n))
    if jt == JoinType.Full:
        assert sorted(x for x, k in zip(lid, both) if not k and x is not None) == list(range(shift))
        assert sorted(x for x, k in zip(rid, both) if not k and x is not None) == list(range(n, n + shift))
    assert lookups >= 1


@pytest.mark.gpu
@pytest.mark.parametrize("jt", [JoinType.Inner, JoinType.Left])
@pytest.mark.parametrize("wide", [False, True])
def test_plan_multi_conjunct_join(ctx, sides, jt, wide):
    """on = a.s = b.s AND a.i = b.i.  `wide`: the Int64 keys spread over 2^62, so the packed key is
    a hash of the tuple and the whole `on` (with its Utf8 comparison) is re-checked."""
    lk, lid, rk, rid = sides
    r = np.random.default_rng(43)
    ivals = np.array([-(1 << 61), -5, 0, 1, 1 << 61], np.int64) if wide else np.arange(5, dtype=np.int64)
    li, ri = ivals[r.integers(0, 5, NL)], ivals[r.integers(0, 5, NR)]
    lmask, rmask = r.random(NL) < 0.03, r.random(NR) < 0.03  # NULL integer components
    lt = pa.table({"s": pa.array(lk, pa.binary()).cast(pa.string(), safe=False), "i": pa.array(li, mask=lmask),
                   "id": pa.array(lid)})
    rt = pa.table({"s": pa.array(rk, pa.binary()).cast(pa.string(), safe=False), "i": pa.array(ri, mask=rmask),
                   "id": pa.array(rid)})
    on = binop(binop(Column("a.s", 0), BinaryOp.Equal, Column("b.s", 3)), BinaryOp.And,
               binop(Column("a.i", 1), BinaryOp.Equal, Column("b.i", 4)))
    t, lookups = run_plan(ctx, HashJoin(Scan(source(lt, "a")), Scan(source(rt, "b")), jt, on))

    def keys(ss, ii, mask):
        return [None if s is None or m else (s, int(i)) for s, i, m in zip(ss, ii, mask)]

    def rows(ss, ii, mask, ids):
        return [(s, None if m else int(i), int(d)) for s, i, m, d in zip(ss, ii, mask, ids)]

    want = py_join(jt, keys(lk, li, lmask), rows(lk, li, lmask, lid), keys(rk, ri, rmask), rows(rk, ri, rmask, rid))
    got = Counter()
    # the strings hold bytes that are not UTF-8: read them back as binary
    cols = [t.column(i).cast(pa.binary()).to_pylist() if i in (0, 3) else t.column(i).to_pylist() for i in range(6)]
    got.update(zip(*cols))
    assert sum(want.values()) > 500
    assert got == want
    assert lookups >= 1, "the string conjunct was not used as a key"
