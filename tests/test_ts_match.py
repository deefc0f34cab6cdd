"""Full-text match (`@@`, QEH_OP_TSMATCH = 13) over operands that may be wrapped in TO_TSVECTOR /
TO_TSQUERY: typing (expr.cpp), the rewrite (k_scalar_fn.hip), the two kernels of k_ts_match.hip
behind qeh_eval / qeh_filter / qeh_ts_match, and plans through QueryExecutor.

Expected values never come from the code under test.  The reference (crates/query-executor/src/
operators.rs:261-318 and :571-610) is restated on `bytes`, unfused: `ref_tsvector` and `ref_tsquery`
materialise the strings the reference's functions return, `ref_match` splits those strings again
as its `@@` does.  The device never builds the strings; its fused evaluation is checked against
the materialising one.  bytes.split() cuts at 0x09-0x0D and 0x20, which is Rust's split_whitespace
on ASCII; bytes.lower() maps ASCII letters only.

Data: row i of a data set is TEMPLATES[i % len(TEMPLATES)] (a few fixed rows are overridden by a
300-byte and a 5000-byte row), so every window of 63 rows or more holds rows of both outcomes for
every query below; each case asserts that on the reference's output (at least 10 % of the non-NULL
rows true and 10 % false) before it looks at the device.  Data sets of 0 and 1 rows cannot hold both
outcomes and are exempt, as are the queries without a term ('' , '&', '!gpu'), true for every row.
The 64- and 65-term queries are both-outcome by the rows they meet: ALL holds every term
(all-present), MISS_63 lacks only t63 -- the highest bit of a 64-term mask -- and MISS_64 only t64
(one-missing).

The plan answers on tests/golden/employees.csv x departments.csv are derived by hand:

    employees   id name    dept_id        departments  dept_id dept_name
                1  Alice   101                         101     Engineering
                2  Bob     102                         102     Sales
                3  Charlie 101                         103     HR
                4  Diana   103                         104     Marketing
                5  Eve     102
                6  Frank   NULL

to_tsvector(name) is the lower-cased name; 'ALICE' under to_tsquery is alice -> Alice; 'ali' is no
whole token -> nobody; 'alice | bob' needs both terms -> nobody; CONCAT(name, ' ', dept_name) of the
inner join holds engineering and charlie only for Charlie (Frank's NULL dept_id does not join).
"""
import ctypes
import os
import re

import numpy as np
import pytest

import qe_hip
from qe_hip import (AggregateFunction as AF, BinaryOp, Filter, HashJoin, JoinType, Literal, MemoryDataSource, Projection,
                    QueryExecutor, ScalarFunction, ScalarFunctionType, ScalarValue, Scan, UnaryExpr, UnaryOp, abi, binop,
                    col, lit)
from qe_hip.device import DeviceColumn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
I64, F64, B, U8 = abi.DT_INT64, abi.DT_FLOAT64, abi.DT_BOOL, abi.DT_UTF8
T, INV, UNS = abi.QEH_E_TYPE, abi.QEH_E_INVALID, abi.QEH_E_UNSUPPORTED
ROWS = [0, 1, 63, 64, 65, 257, 5000]
PLAIN, VEC, QRY = abi.TS_PLAIN, abi.TS_TSVECTOR, abi.TS_TSQUERY
MODES = [PLAIN, VEC, QRY]
MODE_ID = {PLAIN: "plain", VEC: "tsvector", QRY: "tsquery"}


def fn(name, *args):
    return ScalarFunction(getattr(ScalarFunctionType, name), list(args))


def wrap(mode, e):
    return e if mode == PLAIN else fn("ToTsVector" if mode == VEC else "ToTsQuery", e)


def match(doc, query, dmode=PLAIN, qmode=PLAIN):
    return binop(wrap(dmode, doc), BinaryOp.TsMatch, wrap(qmode, query))


# ---- the reference, restated -----------------------------------------------------------------------

def ref_tsvector(s):
    return b" ".join(t.lower() for t in sorted(set(re.findall(rb"[0-9A-Za-z]+", s))))


def ref_tsquery(s):
    return b" ".join(t if t in (b"&", b"|", b"!") else t.lower() for t in s.split())


def ref_side(mode, s):
    return s if mode == PLAIN else (ref_tsvector(s) if mode == VEC else ref_tsquery(s))


def ref_match(doc, query):
    doc_tokens = set(doc.split())
    terms = [t for t in query.split() if t != b"&" and t != b"|" and not t.startswith(b"!")]
    return all(t in doc_tokens for t in terms)


def ref_column(docs, queries, dmode, qmode):
    """queries: one literal (bytes) or a list of per-row bytes."""
    if isinstance(queries, bytes):
        q = ref_side(qmode, queries)
        return np.array([ref_match(ref_side(dmode, d), q) for d in docs], bool)
    return np.array([ref_match(ref_side(dmode, d), ref_side(qmode, q)) for d, q in zip(docs, queries)], bool)


# ---- data ------------------------------------------------------------------------------------------------

TERMS = [b"t%02d" % i for i in range(66)]
ALL = b" ".join(TERMS)
MISS_63 = b" ".join(t for t in TERMS if t != b"t63")
MISS_64 = b"\t".join(t for t in TERMS if t != b"t64")
MIXED = b" gpu.kernel gpu_kernel lds;"  # pieces a tsvector cuts apart: a separator inside and at the end
TEMPLATES = [
    b"gpu kernel", b"GPU Kernel launch", b"gpu\tkernel\nlds", b"the gpu runs" + MIXED, b"kernel only here gpus gp" + MIXED, ALL,
    b"GPU,Kernel;a&b", b"a&b gpu" + MIXED, b"a&b  kernel\x0bgpu", b"gp gpus kernels", b"gpus\rgp\x0ckernel", MISS_63,
    b"x_y gpu_kernel", b"Gpu KERNEL wave64 64", b"", b" \t\n\x0b\x0c\r", b"a", ALL,
    b"!gpu kernel", b"kernel gp", b"u gpu", ALL, b"lds wave64 gpus gp" + MIXED, MISS_64,
    b"gpu Kernel a&b", b"GPU kernel gp", b"gpus gpu kernel GPU Kernel", b"kernel\ngpu", b"GPU  Kernel\tgpu kernel", ALL,
    b"g gp gpus" + MIXED, b"gpu.kernel", b"a & b", b"GPU Kernel", b"gpus kernel a&b gp", ALL,
]
ROW_300 = (b"kernel " * 40 + b"gpu " + b"z" * 16)[:300]
ROW_5000 = b"lds wave64 " * 450 + b"GPU Kernel gpu kernel gp a&b " + b"x" * 21  # the words sit past four steps
assert len(ROW_300) == 300 and len(ROW_5000) == 5000
NON_ASCII = "gpu kernel café a&b".encode()


def make_docs(n):
    docs = [TEMPLATES[i % len(TEMPLATES)] for i in range(n)]
    if n > 9:
        docs[9] = ROW_300
    if n > 40:
        docs[40] = ROW_5000
    return docs


def null_mask(n):
    """Every seventh row NULL, from row 3 (7 and len(TEMPLATES) are coprime: every template is hit)."""
    return np.array([i % 7 != 3 for i in range(n)], bool)


def with_null_bytes(docs, valid):
    """NULL rows keep bytes, every other one non-ASCII: they must not be inspected."""
    out = list(docs)
    for k, i in enumerate(np.flatnonzero(~valid)):
        out[i] = NON_ASCII if k % 2 == 0 else b"gpu kernel a&b " + docs[i]
    return out


Q64 = b" & ".join(TERMS[:64])
Q65 = b" ".join(TERMS[:65])
LITERALS = {
    "empty": b"", "amp": b"&", "gpu": b"gpu", "GPU_and_Kernel": b"GPU & Kernel", "gpu_or_kernel": b"gpu | kernel",
    "not_gpu": b"!gpu", "gpu_not_kernel": b"gpu !kernel", "a_amp_b": b"a&b", "spaces": b"\t gpu \n",
    "prefix": b"gp", "extension": b"gpus", "duplicate": b"kernel gpu kernel", "q64": Q64, "q65": Q65,
}
ALL_TRUE = {"empty", "amp", "not_gpu"}
# terms with a byte that is no letter or digit, inside and at their end: one piece under a plain or
# TO_TSQUERY side, cut apart by TO_TSVECTOR
MIXED_TERMS = {"amp_inside": b"a&b", "dot_inside": b"gpu.kernel", "underscore_inside": b"gpu_kernel",
               "semicolon_at_end": b"lds;"}


def mixed_expectation(dmode, qmode):
    """What a MIXED_TERMS query must give by construction: under a TO_TSVECTOR document no token
    holds such a byte, so a query side that keeps the term whole matches no row ("none"); two sides
    that both keep it whole have rows of both outcomes ("both"); a TO_TSVECTOR query cuts the term
    into alphanumeric terms, the case the other queries of the grid cover ("any")."""
    if qmode == VEC:
        return "any"
    return "none" if dmode == VEC else "both"


def assert_both_outcomes(want, valid, what):
    live = want[valid]
    assert live.sum() * 10 >= len(live) and (~live).sum() * 10 >= len(live), (what, int(live.sum()), len(live))


def test_the_restatement_alone_meets_the_both_outcomes_condition():
    """On the CPU: every (data set, query) the GPU tests assert it for."""
    for n in ROWS[2:]:
        docs = make_docs(n)
        for valid in (np.ones(n, bool), null_mask(n)):
            for name, q in LITERALS.items():
                if name not in ALL_TRUE:
                    assert_both_outcomes(ref_column(docs, q, PLAIN, PLAIN), valid, (n, name))
    for n in (65, 257):
        docs = make_docs(n)
        for dm in MODES:
            for qm in MODES:
                for name in pairing_queries(qm):
                    assert_both_outcomes(ref_column(docs, LITERALS[name], dm, qm), null_mask(n), (n, dm, qm, name))
        for dm in MODES:
            for qm in MODES:
                for name, q in MIXED_TERMS.items():
                    want = ref_column(docs, q, dm, qm)
                    if mixed_expectation(dm, qm) == "both":
                        assert_both_outcomes(want, null_mask(n), (n, dm, qm, name))
                    if mixed_expectation(dm, qm) == "none":
                        assert not want.any()
    # sorted and de-duplicated before lower-casing: "B" < "a" < "b", and the two b's both stay
    assert ref_tsvector(b"b_a B,a  a") == b"b a b" and ref_tsquery(b" A & !B |  c ") == b"a & !b | c"
    assert ref_match(b"a b", b"a | c") is False and ref_match(b"a", b"!b &") is True


def pairing_queries(qmode):
    """Lower-case queries have both outcomes under all nine pairings; an upper-case one only where
    the query side folds (under a plain query against a folding document no term can match)."""
    return ["gpu", "gpu_or_kernel", "prefix", "extension", "q64", "q65"] + (["GPU_and_Kernel"] if qmode != PLAIN else [])


# ---- helpers -----------------------------------------------------------------------------------------

def ty(expr, dtypes):
    lib = qe_hip.load()
    e, keep = expr.to_c()
    d = (ctypes.c_int32 * max(len(dtypes), 1))(*dtypes)
    out = ctypes.c_int32(-1)
    s = lib.qeh_expr_type(d, len(dtypes), ctypes.byref(e), ctypes.byref(out))
    return s, out.value, lib.qeh_last_error().decode()


def upload_slots(ctx, slots, valid=None):
    """A Utf8 column whose row i holds slots[i] whatever its validity (a NULL row may own bytes)."""
    n = len(slots)
    offs = np.zeros(n + 1, np.int32)
    if n:
        offs[1:] = np.cumsum([len(b) for b in slots])
    data = np.frombuffer(b"".join(slots), np.uint8) if offs[-1] else np.zeros(8, np.uint8)
    po, pd = ctx.alloc(offs.nbytes), ctx.alloc(max(data.nbytes, 8))
    ctx.h2d(po, offs)
    ctx.h2d(pd, data)
    c = abi.QehColumn(dtype=U8, owned=0, length=n, offset=0, null_count=0, values=pd, offsets=po,
                      values_bytes=int(offs[-1]))
    bufs = [po, pd]
    if valid is not None:
        valid = np.asarray(valid, bool)
        vb = qe_hip.device.pack_bits(valid)
        q = ctx.alloc(max(vb.nbytes, 8))
        if vb.nbytes:
            ctx.h2d(q, vb)
        c.validity = q
        c.null_count = int(n - valid.sum())
        bufs.append(q)
    return DeviceColumn(ctx, c, bufs)


def sliced(ctx, slots, valid=None):
    """The column of `slots` as rows [3, 3 + n) of a longer one whose first three rows own 3 bytes:
    column offset 3, first offset 3, and the slice's first byte at an odd address."""
    lead = [b"x", b"", b"yz"]
    full = upload_slots(ctx, lead + list(slots), None if valid is None else np.concatenate([[True] * 3, valid]))
    return ctx.slice(full, 3, len(slots))


def evaluate(ctx, cols, expr, n=None):
    r = ctx.eval(cols, expr, n)
    return r[0] if isinstance(r, tuple) else r


def check_bool(out, want, valid, what=""):
    assert out.dtype == B and len(out) == len(want), what
    vals, v = out.to_numpy()
    v = np.ones(len(want), bool) if v is None else v
    assert np.array_equal(v, valid), what
    bad = np.flatnonzero(vals[valid] != want[valid])
    assert len(bad) == 0, (what, bad[:8])


def launches(ctx, call, names):
    ctx.timing(True)
    ctx.timing_reset()
    try:
        result = call()
        return result, {k: ctx.kernel_time(k)[1] for k in names}
    finally:
        ctx.timing(False)


KERNELS = ["ts_match_stream", "ts_match_rows"]


@pytest.fixture(scope="module")
def datasets(ctx):
    """(n, nulls, offset) -> (device column, the slots, validity), uploaded once."""
    cache = {}

    def get(n, nulls, offset):
        key = (n, nulls, offset)
        if key not in cache:
            valid = null_mask(n) if nulls else np.ones(n, bool)
            slots = with_null_bytes(make_docs(n), valid)
            up = sliced if offset else upload_slots
            cache[key] = (up(ctx, slots, valid if nulls else None), slots, valid)
        return cache[key]
    return get


# ---- CPU: the encoding and the typing ---------------------------------------------------------------

def test_header_and_binding_declare_op_13():
    src = open(os.path.join(ROOT, "include", "qeh.h")).read()
    assert "#define QEH_ABI_VERSION 1" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bQEH_OP_TSMATCH\s*=\s*13\b", code) and re.search(r"\bqeh_ts_match\s*\(", code)
    for v, name in enumerate(["PLAIN", "TSVECTOR", "TSQUERY"]):
        assert re.search(r"\bQEH_TS_%s\s*=\s*%d\b" % (name, v), code) and getattr(abi, "TS_" + name) == v
    assert abi.OP_TSMATCH == 13 and BinaryOp.TsMatch == 13 and abi.OP_OR == 12
    assert ctypes.sizeof(abi.QehExprNode) == 40 and qe_hip.load().qeh_abi_version() == 1
    assert "qeh_ts_match" in abi.SIGNATURES and hasattr(qe_hip.load(), "qeh_ts_match")
    e, keep = match(col(0), lit("a b"), VEC, QRY).to_c()
    assert [(e.nodes[i].kind, e.nodes[i].op) for i in range(e.n_nodes)] == [
        (abi.EX_COLUMN, 0), (abi.EX_SCALAR_FUNCTION, abi.FN_TO_TSVECTOR), (abi.EX_LITERAL, 0),
        (abi.EX_SCALAR_FUNCTION, abi.FN_TO_TSQUERY), (abi.EX_BINARY, 13)]


def test_expr_type_is_bool_for_all_nine_pairings():
    for dm in MODES:
        for qm in MODES:
            assert ty(match(col(0), lit("gpu & kernel"), dm, qm), [U8])[:2] == (0, B), (dm, qm)
            assert ty(match(col(0), col(1), dm, qm), [U8, U8])[:2] == (0, B), (dm, qm)
            assert ty(match(lit("a b"), col(0), dm, qm), [U8])[:2] == (0, B), (dm, qm)
    # the match is a Bool operand like any other; a function's Utf8 result is an operand
    assert ty(match(col(0), lit("x"), VEC, QRY) & binop(col(1), BinaryOp.Greater, lit(3)), [U8, I64])[:2] == (0, B)
    assert ty(UnaryExpr(UnaryOp.Not, match(col(0), lit("x"))), [U8])[:2] == (0, B)
    assert ty(match(fn("Concat", col(0), lit(" "), col(1)), lit("x"), VEC, QRY), [U8, U8])[:2] == (0, B)
    assert ty(match(fn("Lower", col(0)), fn("Upper", col(1))), [U8, U8])[:2] == (0, B)


LEFT, RIGHT = "@@ left operand must be tsvector (string)", "@@ right operand must be tsquery (string)"


def test_expr_type_errors_and_their_order():
    cases = [
        (match(col(0), lit("x")), [I64], T, LEFT),
        (match(col(0), col(1)), [U8, I64], T, RIGHT),
        (match(col(0), col(1)), [B, F64], T, LEFT),  # the left downcast fails first
        (match(col(0), lit(True)), [U8], T, RIGHT),
        (match(col(0), Literal(ScalarValue.Utf8(None))), [U8], T, RIGHT),  # a typed NULL is a NullArray
        (match(Literal(ScalarValue.Utf8(None)), col(0)), [U8], T, LEFT),
        (match(lit(None), col(0)), [U8], T, LEFT),
        (match(col(0), lit(None)), [U8], T, RIGHT),
        (match(binop(col(0), BinaryOp.Equal, lit("x")), lit("x")), [U8], T, LEFT),  # a Bool operand
        # the functions: arity, then type
        (match(fn("ToTsVector"), lit("x")), [], INV, "TO_TSVECTOR requires 1 argument"),
        (match(col(0), fn("ToTsQuery")), [U8], INV, "TO_TSQUERY requires 1 argument"),
        (match(fn("ToTsVector", col(0)), lit("x")), [I64], T, "TO_TSVECTOR requires string argument"),
        (match(col(0), fn("ToTsQuery", col(1))), [U8, B], T, "TO_TSQUERY requires string argument"),
        (match(col(0), fn("ToTsQuery", Literal(ScalarValue.Utf8(None)))), [U8], T, "TO_TSQUERY requires string argument"),
        # both operands are evaluated before the match looks at either: the left one's error first
        (match(fn("ToTsVector", col(0)), fn("ToTsQuery")), [I64], T, "TO_TSVECTOR requires string argument"),
        (match(fn("Upper", col(0)), fn("Ceil", col(0))), [I64], T, "UPPER requires string argument"),
        (match(col(0), fn("Ceil", col(0))), [I64], T, "CEIL requires float argument"),  # before "@@ left ..."
        (match(col(0), fn("ToTsQuery")), [I64], INV, "TO_TSQUERY requires 1 argument"),
        (match(col(0), binop(col(0), BinaryOp.Add, lit(1.5))), [I64], T, "Unsupported types for addition"),
        (match(col(3), lit("x")), [U8], INV, "Column index 3 out of bounds"),
    ]
    for expr, dts, status, msg in cases:
        s, _, got = ty(expr, dts)
        assert (s, got) == (status, msg), msg
    # an extra argument is typed and ignored, as for every function
    assert ty(match(fn("ToTsVector", col(0), col(1)), lit("x")), [U8, I64])[:2] == (0, B)


def test_standalone_and_nested_ts_functions_are_refused_as_before():
    vec_msg = "TO_TSVECTOR is not evaluated on the device (Unicode tokenising)"
    qry_msg = "TO_TSQUERY is not evaluated on the device (Unicode tokenising)"
    cases = [
        (fn("ToTsVector", col(0)), vec_msg),
        (fn("ToTsQuery", col(0)), qry_msg),
        (fn("ToTsVector"), vec_msg),  # no arity check either, as before
        (binop(fn("ToTsVector", col(0)), BinaryOp.Equal, lit("x")), vec_msg),
        (fn("Upper", fn("ToTsQuery", col(0))), qry_msg),
        (match(fn("ToTsVector", fn("ToTsVector", col(0))), lit("x")), vec_msg),  # only the direct operand
        (match(col(0), fn("ToTsQuery", fn("ToTsQuery", lit("x")))), qry_msg),
        (match(fn("Upper", fn("ToTsVector", col(0))), lit("x")), vec_msg),
        (match(col(0), fn("Concat", lit("a "), fn("ToTsQuery", col(0)))), qry_msg),
        (match(col(0), lit("x")) & binop(fn("ToTsQuery", col(0)), BinaryOp.Equal, lit("x")), qry_msg),
    ]
    for expr, msg in cases:
        s, _, got = ty(expr, [U8])
        assert (s, got) == (UNS, msg), msg


# ---- GPU: literal queries -------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("name", list(LITERALS))
def test_literal_queries_over_plain_documents(ctx, datasets, name):
    """`doc @@ 'literal'`, both sides as they are: every row count, with and without NULLs, column
    offset 0 and 3.  Up to 64 distinct terms take the stream kernel, 65 the row kernel."""
    q = LITERALS[name]
    for n in ROWS:
        for nulls in (False, True):
            for offset in (0, 3):
                doc, slots, valid = datasets(n, nulls, offset)
                want = ref_column(slots, q, PLAIN, PLAIN)
                if n >= 63 and name not in ALL_TRUE:
                    assert_both_outcomes(want, valid, (n, nulls, name))
                if name in ALL_TRUE:
                    assert want.all()
                out, ran = launches(ctx, lambda: evaluate(ctx, [doc], match(col(0), lit(q)), n), KERNELS)
                check_bool(out, want, valid, (name, n, nulls, offset))
                if n > 0:
                    assert ran == ({"ts_match_stream": 0, "ts_match_rows": 1} if name == "q65" else
                                   {"ts_match_stream": 1, "ts_match_rows": 0}), (name, n, ran)


@pytest.mark.gpu
@pytest.mark.parametrize("qmode", MODES, ids=[MODE_ID[m] for m in MODES])
@pytest.mark.parametrize("dmode", MODES, ids=[MODE_ID[m] for m in MODES])
def test_all_nine_mode_pairings(ctx, datasets, dmode, qmode):
    for n in (65, 257):
        for offset in (0, 3):
            doc, slots, valid = datasets(n, True, offset)
            for name in pairing_queries(qmode):
                q = LITERALS[name]
                want = ref_column(slots, q, dmode, qmode)
                assert_both_outcomes(want, valid, (n, dmode, qmode, name))
                check_bool(evaluate(ctx, [doc], match(col(0), lit(q), dmode, qmode), n), want, valid, (name, n, offset))
                # the same through the row kernel: a query column that repeats the literal
                qcol = upload_slots(ctx, [q] * n)
                check_bool(evaluate(ctx, [doc, qcol], match(col(0), col(1), dmode, qmode), n), want, valid, (name, n, "column"))


@pytest.mark.gpu
@pytest.mark.parametrize("qmode", MODES, ids=[MODE_ID[m] for m in MODES])
@pytest.mark.parametrize("dmode", MODES, ids=[MODE_ID[m] for m in MODES])
def test_terms_with_non_alphanumeric_bytes(ctx, datasets, monkeypatch, dmode, qmode):
    """A term cut by the query's mode may span what the document's mode separates ('a&b', 'gpu.kernel',
    'lds;' against a tsvector whose tokens are a, b, gpu, kernel, lds): it equals no token, although
    the document's bytes hold it between two separators.  The stream kernel, the row kernel and the
    restatement have to agree."""
    for n in (65, 257):
        for offset in (0, 3):
            doc, slots, valid = datasets(n, True, offset)
            for name, q in MIXED_TERMS.items():
                want = ref_column(slots, q, dmode, qmode)
                kind = mixed_expectation(dmode, qmode)
                if kind == "both":
                    assert_both_outcomes(want, valid, (n, dmode, qmode, name))
                if kind == "none":
                    assert not want[valid].any()
                for env, kernel in ((None, "ts_match_stream"), ("1", "ts_match_rows")):
                    if env:
                        monkeypatch.setenv("QEH_NO_TS_STREAM", env)
                    else:
                        monkeypatch.delenv("QEH_NO_TS_STREAM", raising=False)
                    out, ran = launches(ctx, lambda: evaluate(ctx, [doc], match(col(0), lit(q), dmode, qmode), n), KERNELS)
                    assert ran[kernel] == 1 and sum(ran.values()) == 1
                    check_bool(out, want, valid, (name, n, offset, kernel))
    monkeypatch.delenv("QEH_NO_TS_STREAM", raising=False)


@pytest.mark.gpu
def test_the_forced_row_kernel_agrees(ctx, datasets, monkeypatch):
    monkeypatch.setenv("QEH_NO_TS_STREAM", "1")
    doc, slots, valid = datasets(5000, True, 3)
    for name in ("GPU_and_Kernel", "q64", "empty"):
        for dm, qm in ((PLAIN, PLAIN), (VEC, QRY)):
            want = ref_column(slots, LITERALS[name], dm, qm)
            out, ran = launches(ctx, lambda: evaluate(ctx, [doc], match(col(0), lit(LITERALS[name]), dm, qm), 5000), KERNELS)
            assert ran == {"ts_match_stream": 0, "ts_match_rows": 1}
            check_bool(out, want, valid, name)


@pytest.mark.gpu
def test_a_literal_beyond_the_term_table_takes_the_row_kernel(ctx):
    """The stream kernel's table holds 2048 term bytes: a 3000-byte term goes to the row kernel, the
    same bytes behind '!' are no term and stay on the stream kernel."""
    long = b"Z" * 3000
    docs = make_docs(65)
    docs[1] = long + b" gpu"
    docs[2] = long[:-1] + b" gpu"
    doc = upload_slots(ctx, docs)
    for q, kernel in ((b"gpu " + long, "ts_match_rows"), (b"gpu !" + long, "ts_match_stream")):
        for dm, qm in ((PLAIN, PLAIN), (VEC, QRY)):
            want = ref_column(docs, q, dm, qm)
            assert want[1] and (want[2] == (kernel == "ts_match_stream"))
            out, ran = launches(ctx, lambda: evaluate(ctx, [doc], match(col(0), lit(q), dm, qm), 65), KERNELS)
            assert ran[kernel] == 1 and sum(ran.values()) == 1
            check_bool(out, want, np.ones(65, bool), (kernel, dm, qm))


# ---- GPU: query columns, literal documents ---------------------------------------------------------

def query_slots(n):
    cycle = [b"gpu", b"GPU & Kernel", b"", b"kernel | gpu", b"!gpu kernel", b"a&b", b"gp", b" \t", b"gpus gp", b"t00 t65",
             b"lds", b"kernel"]
    return [cycle[(i // 3) % len(cycle)] for i in range(n)]  # changes every third row: out of step with the documents


@pytest.mark.gpu
@pytest.mark.parametrize("dmode,qmode", [(PLAIN, PLAIN), (VEC, QRY), (QRY, VEC)], ids=["plain", "vec_qry", "qry_vec"])
def test_a_query_column_with_its_own_nulls(ctx, datasets, dmode, qmode):
    for n in ROWS:
        doc, slots, valid = datasets(n, True, 3)
        qs = query_slots(n)
        qvalid = np.array([i % 5 != 1 for i in range(n)], bool)
        qs_dev = [NON_ASCII if not v else s for s, v in zip(qs, qvalid)]  # NULL queries own bytes too
        want = ref_column(slots, qs, dmode, qmode)
        both = valid & qvalid
        if n >= 63:
            assert_both_outcomes(want, both, (n, dmode, qmode))
        for up in (upload_slots, sliced):
            out = evaluate(ctx, [doc, up(ctx, qs_dev, qvalid)], match(col(0), col(1), dmode, qmode), n)
            check_bool(out, want, both, (n, dmode, qmode))


@pytest.mark.gpu
def test_a_literal_document_against_a_query_column(ctx):
    for n in (1, 65, 257):
        qs = query_slots(n)
        qvalid = np.array([i % 5 != 1 for i in range(n)], bool)
        d = b"the GPU kernel, a&b and gp"
        for dm, qm in ((PLAIN, PLAIN), (VEC, QRY), (VEC, PLAIN)):
            want = ref_column([d] * n, qs, dm, qm)
            if n >= 63:
                assert_both_outcomes(want, qvalid, (n, dm, qm))
            out = evaluate(ctx, [upload_slots(ctx, qs, qvalid)], match(lit(d), col(0), dm, qm), n)
            check_bool(out, want, qvalid, (n, dm, qm))
    # two literals: one answer broadcast over the rows
    out = evaluate(ctx, [ctx.upload(np.arange(70))], match(lit("GPU kernel"), lit("gpu & KERNEL"), VEC, QRY), 70)
    check_bool(out, np.ones(70, bool), np.ones(70, bool))
    out = evaluate(ctx, [ctx.upload(np.arange(70))], match(lit("GPU kernel"), lit("gpu & KERNEL")), 70)
    check_bool(out, np.zeros(70, bool), np.ones(70, bool))


@pytest.mark.gpu
def test_context_ts_match_is_the_c_entry_point(ctx, datasets):
    doc, slots, valid = datasets(257, True, 3)
    check_bool(ctx.ts_match(doc, "GPU & Kernel", VEC, QRY), ref_column(slots, b"GPU & Kernel", VEC, QRY), valid)
    check_bool(ctx.ts_match(doc, b"a&b"), ref_column(slots, b"a&b", PLAIN, PLAIN), valid)
    qs = query_slots(257)
    check_bool(ctx.ts_match(doc, upload_slots(ctx, qs), VEC, QRY), ref_column(slots, qs, VEC, QRY), valid)
    with pytest.raises(qe_hip.QehError) as err:
        ctx.ts_match(ctx.upload(np.arange(257)), "gpu")
    assert err.value.status == T and err.value.message == LEFT
    with pytest.raises(qe_hip.QehError) as err:
        ctx.ts_match(doc, upload_slots(ctx, qs[:10]))
    assert err.value.status == INV


# ---- GPU: non-ASCII ------------------------------------------------------------------------------------

@pytest.mark.gpu
def test_non_ascii_is_refused_in_valid_rows_only(ctx):
    n = 130
    docs = make_docs(n)
    valid = null_mask(n)
    qs = query_slots(n)

    def refused(call):
        with pytest.raises(qe_hip.QehError) as err:
            call()
        assert err.value.status == UNS and "@@" in err.value.message and "non-ASCII" in err.value.message

    for row in (0, 64, 128):  # valid rows (none is 3 mod 7); 128 is the first of a wave of two
        assert valid[row]
        bad = list(docs)
        bad[row] = docs[row] + b" \xc3\xa9"
        for up in (upload_slots, sliced):
            for dm, qm in ((PLAIN, PLAIN), (VEC, QRY)):
                refused(lambda: evaluate(ctx, [up(ctx, bad, valid)], match(col(0), lit("gpu"), dm, qm), n))
                refused(lambda: evaluate(ctx, [up(ctx, bad, valid), upload_slots(ctx, qs)], match(col(0), col(1), dm, qm), n))
                refused(lambda: evaluate(ctx, [upload_slots(ctx, docs), up(ctx, bad, valid)], match(col(0), col(1), dm, qm), n))
                # a non-NULL row of either side counts, also opposite a NULL row of the other side
                other = np.ones(n, bool)
                other[row] = False
                refused(lambda: evaluate(ctx, [up(ctx, bad, valid), upload_slots(ctx, qs, other)], match(col(0), col(1), dm, qm), n))
                refused(lambda: evaluate(ctx, [upload_slots(ctx, docs, other), up(ctx, bad, valid)], match(col(0), col(1), dm, qm), n))
    refused(lambda: evaluate(ctx, [upload_slots(ctx, docs)], match(col(0), lit("café"), VEC, QRY), n))
    refused(lambda: evaluate(ctx, [upload_slots(ctx, qs)], match(lit("café gpu"), col(0)), n))
    # the same bytes in NULL rows only are accepted (with_null_bytes puts them there)
    hidden = with_null_bytes(docs, valid)
    assert any(b"\xc3" in s for s in hidden)
    for dm, qm in ((PLAIN, PLAIN), (VEC, QRY)):
        out = evaluate(ctx, [sliced(ctx, hidden, valid)], match(col(0), lit("gpu"), dm, qm), n)
        check_bool(out, ref_column(docs, b"gpu", dm, qm), valid)
        out = evaluate(ctx, [upload_slots(ctx, docs), upload_slots(ctx, hidden, valid)], match(col(0), col(1), dm, qm), n)
        check_bool(out, ref_column(docs, hidden, dm, qm), valid)


# ---- GPU: through filter, eval, functions and the fused entry points --------------------------------

@pytest.mark.gpu
def test_filter_and_filter_limit_combine_the_match_with_other_terms(ctx, datasets):
    n = 5000
    doc, slots, valid = datasets(n, True, 3)
    ids = np.arange(n)
    m = ref_column(slots, b"GPU & Kernel", VEC, QRY) & valid
    lds = ref_column(slots, b"lds", VEC, QRY) & valid
    has = match(col(0), lit("GPU & Kernel"), VEC, QRY)
    cases = [
        (has, m),
        (has & binop(col(1), BinaryOp.Less, lit(2000)), m & (ids < 2000)),
        (has | match(col(0), lit("lds"), VEC, QRY), m | lds),
        # NOT of a NULL is NULL: dropped
        (UnaryExpr(UnaryOp.Not, has) & binop(col(1), BinaryOp.GreaterEqual, lit(100)), ~m & valid & (ids >= 100)),
    ]
    for pred, keep in cases:
        want = ids[keep]
        assert 0 < len(want) < n
        out, rows = ctx.filter([doc, ctx.upload(ids)], pred, out_idx=[1])
        assert rows == len(want) and np.array_equal(out[0].to_numpy()[0], want)
        out, rows = ctx.filter([doc, ctx.upload(ids)], pred, out_idx=[1, 0], max_rows=7)
        assert rows == 7 and np.array_equal(out[0].to_numpy()[0], want[:7])
        assert out[1].to_bytes() == [slots[i] for i in want[:7]]


@pytest.mark.gpu
def test_eval_projects_the_match_as_a_nullable_bool(ctx, datasets):
    doc, slots, valid = datasets(257, True, 0)
    ids = np.arange(257)
    m = ref_column(slots, b"kernel", QRY, QRY)
    out = evaluate(ctx, [doc, ctx.upload(ids)], match(col(0), lit("kernel"), QRY, QRY) & binop(col(1), BinaryOp.Greater, lit(-1)))
    check_bool(out, m, valid)
    out = evaluate(ctx, [doc], UnaryExpr(UnaryOp.Not, match(col(0), lit("kernel"), QRY, QRY)))
    check_bool(out, ~m, valid)
    doc, slots, valid = datasets(257, False, 3)  # no NULLs anywhere: no validity needed, all rows answer
    out = evaluate(ctx, [doc], match(col(0), lit("kernel"), QRY, QRY))
    check_bool(out, ref_column(slots, b"kernel", QRY, QRY), valid)


@pytest.mark.gpu
def test_a_non_leaf_operand_is_evaluated_first(ctx):
    n = 257
    a = [TEMPLATES[i % len(TEMPLATES)] for i in range(n)]
    b = [TEMPLATES[(i * 5 + 1) % len(TEMPLATES)] for i in range(n)]
    ca, cb = upload_slots(ctx, a), upload_slots(ctx, b)
    both = [x + b" " + y for x, y in zip(a, b)]
    want = ref_column(both, b"gpu & Kernel", VEC, QRY)
    assert_both_outcomes(want, np.ones(n, bool), "concat")
    out = evaluate(ctx, [ca, cb], match(fn("Concat", col(0), lit(" "), col(1)), lit("gpu & Kernel"), VEC, QRY), n)
    check_bool(out, want, np.ones(n, bool))
    # without the separator the two rows' edge words join: CONCAT's bytes, not the rows', are tokenised
    glued = [x + y for x, y in zip(a, b)]
    out = evaluate(ctx, [ca, cb], match(fn("Concat", col(0), col(1)), lit("gpu"), VEC, QRY), n)
    check_bool(out, ref_column(glued, b"gpu", VEC, QRY), np.ones(n, bool))
    # both sides functions of columns: LOWER(a) @@ to_tsquery(b)
    out = evaluate(ctx, [ca, upload_slots(ctx, query_slots(n))], match(fn("Lower", col(0)), col(1), PLAIN, QRY), n)
    check_bool(out, ref_column([x.lower() for x in a], query_slots(n), PLAIN, QRY), np.ones(n, bool))
    # an operand's own error comes before the match's
    with pytest.raises(qe_hip.QehError) as err:
        evaluate(ctx, [ca, ctx.upload(np.arange(n))], match(col(0), binop(col(1), BinaryOp.Divide, lit(0))), n)
    assert err.value.status == abi.QEH_E_DIV0
    with pytest.raises(qe_hip.QehError) as err:
        evaluate(ctx, [ca, ctx.upload(np.arange(n))], match(col(0), col(1)), n)
    assert err.value.status == T and err.value.message == RIGHT
    with pytest.raises(qe_hip.QehError) as err:
        evaluate(ctx, [ca], fn("ToTsVector", col(0)), n)
    assert err.value.status == UNS and "TO_TSVECTOR" in err.value.message
    with pytest.raises(qe_hip.QehError) as err:
        evaluate(ctx, [ca], match(fn("ToTsVector"), lit("x")), n)
    assert (err.value.status, err.value.message) == (INV, "TO_TSVECTOR requires 1 argument")


@pytest.mark.gpu
def test_fused_entry_points_refuse_the_match_by_name(ctx):
    k = ctx.upload(np.arange(100) % 7)
    s = upload_slots(ctx, [b"gpu kernel"] * 100)
    with pytest.raises(qe_hip.QehError) as err:
        ctx.filter_aggregate([k, s], match(col(1), lit("gpu")), [0], [qe_hip.agg(AF.Count, 0)])
    assert err.value.status == UNS and "QEH_OP_TSMATCH" in err.value.message and "@@" in err.value.message
    with pytest.raises(qe_hip.QehError) as err:  # with wrapped operands too: the match is named, not its parts
        ctx.filter_aggregate([k, s], match(col(1), lit("gpu"), VEC, QRY) & binop(col(0), BinaryOp.Less, lit(5)), [0],
                             [qe_hip.agg(AF.Count, 0)])
    assert err.value.status == UNS and "QEH_OP_TSMATCH" in err.value.message


# ---- GPU: plans over employees x departments ------------------------------------------------------------

ID, NAME, AGE, SALARY, DEPT = range(5)
D_ID, D_NAME = 5, 6  # departments' columns after a join with the five employee columns


@pytest.fixture(scope="module")
def srcs():
    import pyarrow.csv as pacsv
    emp = pacsv.read_csv(os.path.join(GOLD, "employees.csv"))  # "NULL" is read as a NULL
    dep = pacsv.read_csv(os.path.join(GOLD, "departments.csv"))
    assert emp["dept_id"].null_count == 1 and emp["name"].null_count == 0
    return (MemoryDataSource(emp.schema, emp.to_batches()), MemoryDataSource(dep.schema, dep.to_batches()))


def column(batches, i=0):
    return [v for b in batches for v in b.column(i).to_pylist()]


@pytest.mark.gpu
@pytest.mark.parametrize("no_fusion", [False, True], ids=["fused", "no_fusion"])
def test_plans_with_a_full_text_predicate(ctx, srcs, monkeypatch, no_fusion):
    emp, dep = srcs
    if no_fusion:
        monkeypatch.setenv("QEH_NO_FUSION", "1")
    ex = QueryExecutor(ctx)

    def names_matching(query):
        return column(ex.execute(Filter(Scan(emp), match(col(NAME), lit(query), VEC, QRY))), NAME)

    assert names_matching("ALICE") == ["Alice"]
    assert names_matching("ali") == []
    assert names_matching("alice | bob") == []
    joined = HashJoin(Scan(emp), Scan(dep), JoinType.Inner, binop(col(DEPT), BinaryOp.Equal, col(D_ID)))
    both = match(fn("Concat", col(NAME), lit(" "), col(D_NAME)), lit("engineering & charlie"), VEC, QRY)
    assert column(ex.execute(Filter(joined, both)), NAME) == ["Charlie"]
    # a Projection of the match: Frank's name is not NULL, so his row is false, not NULL
    plan = Projection(Scan(emp), [col(NAME), match(col(NAME), lit("frank | FRANK"), VEC, QRY),
                                  match(col(NAME), lit("Eve"))], ["name", "is_frank", "is_eve"])
    (b,) = ex.execute(plan)
    assert [str(f.type) for f in b.schema] == ["string", "bool", "bool"]
    assert b.column(1).to_pylist() == [False, False, False, False, False, True]
    assert b.column(2).to_pylist() == [False, False, False, False, True, False]
    # the fusions step around it: HashAggregate(Filter(X)) with the match in the predicate
    from qe_hip import AggregateExpr, HashAggregate
    plan = HashAggregate(Filter(Scan(emp), UnaryExpr(UnaryOp.Not, match(col(NAME), lit("bob"), VEC, QRY))), [col(DEPT)],
                         [AggregateExpr(AF.Count, col(ID))])
    (b,) = ex.execute(plan)
    got = sorted(zip(column([b], 0), column([b], 1)), key=lambda r: (r[0] is None, r[0]))
    assert got == [(101, 2), (102, 1), (103, 1), (None, 1)]
