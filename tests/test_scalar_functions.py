"""Scalar functions in expressions (QEH_EX_SCALAR_FUNCTION): typing (expr.cpp), the kernels of
k_scalar_fn.hip behind qeh_eval / qeh_filter, and plans through QueryExecutor.

Expected values never come from the code under test: `ref_*` below restate evaluate_scalar_function
(crates/query-executor/src/operators.rs:64-259) in Python -- bytes.upper / bytes.lower (ASCII only,
as the device; non-ASCII input must be refused), math.ceil / floor / sqrt with IEEE's signed zeros,
a half-away-from-zero round built from floor and the exact fraction, math.pow, and CONCAT's slot
rule (value(i) of every argument, validity ignored).  The plan answers on tests/golden/employees.csv
x departments.csv are derived by hand:

    employees   id name    age salary dept_id        departments  dept_id dept_name
                1  Alice   25  75000  101                         101     Engineering
                2  Bob     30  85000  102                         102     Sales
                3  Charlie 35  95000  101                         103     HR
                4  Diana   28  80000  103                         104     Marketing
                5  Eve     32  90000  102
                6  Frank   29  78000  NULL

salary is Int64 in the CSV; the reference has no arithmetic coercion (Int64 / Float64 is its type
error), so ROUND(salary / 7.0) reads a Float64 copy of the column appended as `salary_f`.
"""
import ctypes
import math
import os
import re
import zlib

import numpy as np
import pytest

import qe_hip
from qe_hip import (AggregateExpr, AggregateFunction as AF, BinaryOp, Filter, HashAggregate, HashJoin, JoinType,
                    Limit, Literal, MemoryDataSource, Projection, QueryExecutor, ScalarValue, Scan, Sort, UnaryExpr,
                    UnaryOp, abi, binop, col, lit)
from qe_hip.device import DeviceColumn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

I64, F64, I32, F32, B, U8 = abi.DT_INT64, abi.DT_FLOAT64, abi.DT_INT32, abi.DT_FLOAT32, abi.DT_BOOL, abi.DT_UTF8
INT64_MIN, INT64_MAX = -(1 << 63), (1 << 63) - 1
ROWS = [0, 1, 63, 64, 65, 257, 5000]  # a validity-word edge, a partial wave, several blocks

# the largest distance from math.pow measured over power_inputs() on an MI355X, 1 ULP (DESIGN.md §5
# "Scalar functions"), plus 1 ULP of margin for other ROCm point releases
POWER_ULP_BOUND = 2


def fn(name, *args):
    from qe_hip import ScalarFunction, ScalarFunctionType
    return ScalarFunction(getattr(ScalarFunctionType, name), list(args))


# ---- the reference, restated -----------------------------------------------------------------------

def ref_ceil(x):
    if not math.isfinite(x):
        return x
    r = float(math.ceil(x))
    return math.copysign(0.0, x) if r == 0 else r  # ceil(-0.5) = -0.0


def ref_floor(x):
    if not math.isfinite(x):
        return x
    r = float(math.floor(x))
    return math.copysign(0.0, x) if r == 0 else r


def ref_round(x):
    """f64::round: half away from zero.  a - floor(a) is exact (a < 1: floor is 0; else the two are
    within a factor of two), so the tie test is exact."""
    if not math.isfinite(x):
        return x
    a = abs(x)
    f = float(math.floor(a))
    return math.copysign(f + 1.0 if a - f >= 0.5 else f, x)


def ref_sqrt(x):
    if math.isnan(x) or x == math.inf:
        return x
    return math.sqrt(x) if x >= 0 else math.nan  # sqrt(-0.0) = -0.0


def ref_pow(b, e):
    try:
        return math.pow(b, e)
    except OverflowError:
        return math.inf
    except ValueError:  # a negative base with a non-integer exponent
        return math.nan


def ref_abs_i64(x):
    x = int(x)
    return INT64_MIN if x == INT64_MIN else abs(x)  # i64::abs wraps in a release build


REF_F64 = {"Abs": abs, "Ceil": ref_ceil, "Floor": ref_floor, "Round": ref_round, "Sqrt": ref_sqrt}


def ref_concat(columns, n):
    """columns: per argument either a list of n slots (bytes, validity ignored) or one literal bytes."""
    return [b"".join(c if isinstance(c, bytes) else c[i] for c in columns) for i in range(n)]


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
    column offset 3, and the slice's first byte at an odd address."""
    lead = [b"x", b"", b"yz"]
    full = upload_slots(ctx, lead + list(slots), None if valid is None else np.concatenate([[True] * 3, valid]))
    return ctx.slice(full, 3, len(slots))


def evaluate(ctx, cols, expr, n=None):
    r = ctx.eval(cols, expr, n)
    return r[0] if isinstance(r, tuple) else r


def validity(col):
    v = col.to_numpy()[1]
    return np.ones(len(col), bool) if v is None else v


def launches(ctx, call, names):
    ctx.timing(True)
    ctx.timing_reset()
    try:
        result = call()
        return result, {k: ctx.kernel_time(k)[1] for k in names}
    finally:
        ctx.timing(False)


EDGE = b"@AZ[`az{\x7f"  # the SWAR range edges: one below / first / last / one above each letter range, and 0x7F
ALPHABET = np.frombuffer(EDGE + b"MmqQ 09_-.", np.uint8)
LENGTHS = [0, 1, 15, 16, 17, 63, 64, 65]


def make_slots(n, seed):
    """n strings cycling through LENGTHS, one of them 1000 bytes, over ALPHABET; EDGE leads when it fits."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(n):
        ln = 1000 if i == 9 else LENGTHS[i % len(LENGTHS)]
        b = ALPHABET[rng.integers(0, len(ALPHABET), ln)].tobytes()
        if ln >= len(EDGE):
            b = EDGE + b[len(EDGE):]
        out.append(b)
    return out


def null_mask(n, seed):
    v = np.random.default_rng(seed).random(n) > 0.3
    if n > 2:
        v[1], v[2] = False, True  # at least one of each; row 1 (and others) keep a non-empty slot
    return v


# ---- CPU: the encoding -------------------------------------------------------------------------------

FUNCS = ["UPPER", "LOWER", "LENGTH", "CONCAT", "SUBSTRING", "TRIM", "REPLACE", "ABS", "CEIL", "FLOOR", "ROUND", "SQRT",
         "POWER", "COALESCE", "NULLIF", "TO_TSVECTOR", "TO_TSQUERY"]


def test_header_and_binding_declare_the_kind_and_the_function_order():
    src = open(os.path.join(ROOT, "include", "qeh.h")).read()
    assert "#define QEH_ABI_VERSION 1" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bQEH_EX_SCALAR_FUNCTION\s*=\s*8\b", code)
    for v, name in enumerate(FUNCS):
        assert re.search(r"\bQEH_FN_%s\s*=\s*%d\b" % (name, v), code), name
        assert getattr(abi, "FN_" + name) == v
    assert abi.EX_SCALAR_FUNCTION == 8
    assert ctypes.sizeof(abi.QehExprNode) == 40 and qe_hip.load().qeh_abi_version() == 1
    t = qe_hip.ScalarFunctionType
    assert [t.Upper, t.Lower, t.Length, t.Concat, t.Substring, t.Trim, t.Replace, t.Abs, t.Ceil, t.Floor, t.Round,
            t.Sqrt, t.Power, t.Coalesce, t.Nullif, t.ToTsVector, t.ToTsQuery] == list(range(17))


def test_to_c_emits_the_arguments_then_the_node():
    e, keep = fn("Power", binop(col(0), BinaryOp.Add, lit(1.0)), lit(2.0)).to_c()
    assert [e.nodes[i].kind for i in range(e.n_nodes)] == [abi.EX_COLUMN, abi.EX_LITERAL, abi.EX_BINARY, abi.EX_LITERAL,
                                                           abi.EX_SCALAR_FUNCTION]
    assert e.nodes[4].op == abi.FN_POWER and e.nodes[4].index == 2
    e, keep = fn("Upper").to_c()
    assert e.n_nodes == 1 and e.nodes[0].kind == 8 and e.nodes[0].op == abi.FN_UPPER and e.nodes[0].index == 0
    e, keep = fn("Concat", col(1), lit("-"), fn("Lower", col(0))).to_c()
    assert [(e.nodes[i].kind, e.nodes[i].op, e.nodes[i].index) for i in (3, 4)] == [(8, abi.FN_LOWER, 1), (8, abi.FN_CONCAT, 3)]


def test_expr_type_of_functions():
    assert ty(fn("Length", col(0)), [U8])[:2] == (0, I64)
    assert ty(fn("Upper", col(0)), [U8])[:2] == (0, U8)
    assert ty(fn("Lower", lit("Ab")), [])[:2] == (0, U8)
    assert ty(fn("Concat", col(0), lit("x"), col(1)), [U8, U8])[:2] == (0, U8)
    assert ty(fn("Abs", col(0)), [I64])[:2] == (0, I64)
    assert ty(fn("Abs", col(0)), [F64])[:2] == (0, F64)
    for f in ("Ceil", "Floor", "Round", "Sqrt"):
        assert ty(fn(f, col(0)), [F64])[:2] == (0, F64), f
    assert ty(fn("Power", col(0), lit(2.0)), [F64])[:2] == (0, F64)
    for t in (I64, U8, B, I32):
        assert ty(fn("Coalesce", col(0), col(1)), [t, F64])[:2] == (0, t)
    assert ty(binop(fn("Upper", col(0)), BinaryOp.Equal, lit("X")), [U8])[:2] == (0, B)
    assert ty(binop(fn("Abs", binop(col(0), BinaryOp.Subtract, col(1))), BinaryOp.Add, lit(1)), [I64, I64])[:2] == (0, I64)
    assert ty(binop(fn("Length", fn("Concat", col(0), col(1))), BinaryOp.Greater, lit(3)), [U8, U8])[:2] == (0, B)
    # extra arguments are evaluated (typed) and ignored
    assert ty(fn("Sqrt", col(0), col(1)), [F64, U8])[:2] == (0, F64)


def test_expr_type_errors_are_the_references():
    T, INV, UNS = abi.QEH_E_TYPE, abi.QEH_E_INVALID, abi.QEH_E_UNSUPPORTED
    cases = [
        (fn("Ceil", col(0)), [I64], T, "CEIL requires float argument"),
        (fn("Abs", col(0)), [I32], T, "ABS requires numeric argument"),
        (fn("Abs", col(0)), [F32], T, "ABS requires numeric argument"),
        (fn("Power", col(0), lit(2)), [F64], T, "POWER requires float arguments"),
        (fn("Upper", col(0)), [I64], T, "UPPER requires string argument"),
        (fn("Length", col(0)), [F64], T, "LENGTH requires string argument"),
        (fn("Concat", col(0), col(1)), [U8, I64], T, "CONCAT requires string arguments"),
        (fn("Upper"), [], INV, "UPPER requires 1 argument"),
        (fn("Power"), [], INV, "POWER requires 2 arguments"),
        (fn("Power", col(0)), [F64], INV, "POWER requires 2 arguments"),
        (fn("Coalesce"), [], INV, "COALESCE requires at least 1 argument"),
        (fn("Concat"), [], INV, "CONCAT requires at least 1 argument"),
        (fn("Nullif", col(0), col(0)), [I64], UNS, "Nullif function not yet fully implemented"),
        (fn("Substring", col(0)), [U8], UNS, "Substring function not yet fully implemented"),
        (fn("Trim", col(0)), [U8], UNS, "Trim function not yet fully implemented"),
        (fn("Replace", col(0)), [U8], UNS, "Replace function not yet fully implemented"),
    ]
    for expr, dts, status, msg in cases:
        s, _, got = ty(expr, dts)
        assert (s, got) == (status, msg), msg
    s, _, msg = ty(fn("ToTsVector", col(0)), [U8])
    assert s == UNS and "TO_TSVECTOR" in msg
    # an argument's own error comes first, also for an argument the function then ignores
    s, _, msg = ty(fn("Coalesce", col(0), binop(col(0), BinaryOp.Multiply, lit(1.5))), [I64])
    assert (s, msg) == (T, "Unsupported types for multiplication")
    s, _, msg = ty(binop(fn("Upper", col(0)), BinaryOp.Equal, lit(1)), [U8])
    assert s == T and "Invalid comparison operation: Utf8 == Int64" in msg


def test_expressions_without_a_function_type_as_before():
    assert ty(binop(col(0), BinaryOp.Greater, lit(25)), [F64])[:2] == (0, B)
    assert ty(binop(col(0), BinaryOp.Add, lit(1)), [I64])[:2] == (0, I64)
    s, _, msg = ty(binop(col(0), BinaryOp.Multiply, lit(1.1)), [I64])
    assert (s, msg) == (abi.QEH_E_TYPE, "Unsupported types for multiplication")
    s, _, msg = ty(col(3), [I64])
    assert (s, msg) == (abi.QEH_E_INVALID, "Column index 3 out of bounds")
    assert ty(binop(col(0), BinaryOp.Equal, col(1)), [F32, I64])[:2] == (0, B)


def test_operators_over_a_function_type_by_the_operator_rules():
    """The unary / binary typing that compile_expr and the function-aware typing share, reached
    through an expression that holds a function."""
    T = abi.QEH_E_TYPE
    cases = [
        (UnaryExpr(UnaryOp.Not, fn("Abs", col(0))), [I64], "NOT operator requires boolean array"),
        (UnaryExpr(UnaryOp.Minus, fn("Upper", col(0))), [U8], "Unsupported type for negation"),
        (binop(fn("Abs", col(0)), BinaryOp.Add, lit(1.5)), [I64], "Unsupported types for addition"),
        (binop(fn("Sqrt", col(0)), BinaryOp.Modulo, lit(2.0)), [F64], "Modulo operation requires integer arrays"),
        (binop(fn("Length", col(0)), BinaryOp.And, lit(True)), [U8], "AND requires boolean arrays"),
    ]
    for expr, dts, msg in cases:
        s, _, got = ty(expr, dts)
        assert (s, got) == (T, msg), msg
    assert ty(UnaryExpr(UnaryOp.Minus, fn("Abs", col(0))), [F64])[:2] == (0, F64)
    assert ty(UnaryExpr(UnaryOp.Not, binop(fn("Length", col(0)), BinaryOp.Less, lit(3))), [U8])[:2] == (0, B)
    assert ty(binop(fn("Length", col(0)), BinaryOp.Less, col(1)), [U8, F64])[:2] == (0, B)  # Int64 against Float64 coerces


def test_a_typed_null_literal_argument_is_a_null_array():
    """create_literal_array (operators.rs:322-346) has arms for Some(v) only: Utf8(None) or Int64(None)
    falls to the NullArray arm, so the function's downcast fails with its argument-type error."""
    T = abi.QEH_E_TYPE
    s, _, msg = ty(fn("Upper", Literal(ScalarValue.Utf8(None))), [])
    assert (s, msg) == (T, "UPPER requires string argument")
    s, _, msg = ty(fn("Abs", Literal(ScalarValue.Int64(None))), [])
    assert (s, msg) == (T, "ABS requires numeric argument")
    s, _, msg = ty(fn("Concat", col(0), Literal(ScalarValue.Utf8(None))), [U8])
    assert (s, msg) == (T, "CONCAT requires string arguments")


# ---- GPU: numeric ------------------------------------------------------------------------------------

F64_SPECIALS = np.array([0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.49999999999999994, -0.49999999999999994,
                         2.0 ** 52 + 1, -(2.0 ** 52 + 1), -1.0, 1.0, 2.0, 1e300, -1e-300, 5e-324, math.nan, math.inf,
                         -math.inf, 3.999999999999999, -7.000000000000001, 1e15 + 0.5])
I64_SPECIALS = np.array([INT64_MIN, -1, 0, 1, INT64_MAX, INT64_MIN + 1, -123456789012345, 42], np.int64)


def fill(specials, n, seed):
    rng = np.random.default_rng(seed)
    if specials.dtype == np.int64:
        extra = rng.integers(-10 ** 12, 10 ** 12, max(n - len(specials), 0))
    else:
        extra = (rng.random(max(n - len(specials), 0)) - 0.5) * 10.0 ** rng.integers(-3, 6, max(n - len(specials), 0))
    return np.concatenate([specials, extra]).astype(specials.dtype)[:n]


def same_bits(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.int64), want[~nan].view(np.int64))


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [0, 3], ids=["off0", "off3"])
@pytest.mark.parametrize("nulls", [False, True], ids=["nonull", "nulls"])
def test_float_functions_are_bit_exact(ctx, nulls, offset):
    for n in ROWS:
        x = fill(F64_SPECIALS, n, 7 + n)
        valid = null_mask(n, n) if nulls else None
        c = ctx.upload(x, valid, offset=offset)
        for name, ref in REF_F64.items():
            (out, ran) = launches(ctx, lambda: evaluate(ctx, [c], fn(name, col(0))), ["scalar_math", "eval"])
            assert out.dtype == F64 and len(out) == n
            assert ran == {"scalar_math": 1 if n else 0, "eval": 0}
            got, gv = out.to_numpy()
            want = np.array([ref(float(v)) for v in x], np.float64)
            keep = valid if nulls else np.ones(n, bool)
            assert np.array_equal(validity(out), keep), (name, n)
            assert same_bits(got[keep], want[keep]), (name, n)


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [0, 3], ids=["off0", "off3"])
@pytest.mark.parametrize("nulls", [False, True], ids=["nonull", "nulls"])
def test_abs_int64_wraps_at_int64_min(ctx, nulls, offset):
    for n in ROWS:
        x = fill(I64_SPECIALS, n, 11 + n)
        valid = null_mask(n, n + 1) if nulls else None
        out = evaluate(ctx, [ctx.upload(x, valid, offset=offset)], fn("Abs", col(0)))
        assert out.dtype == I64 and len(out) == n
        keep = valid if nulls else np.ones(n, bool)
        assert np.array_equal(validity(out), keep)
        want = np.array([ref_abs_i64(v) for v in x], np.int64)
        assert np.array_equal(out.to_numpy()[0][keep], want[keep])


def power_inputs(n, seed):
    rng = np.random.default_rng(seed)
    b = np.array([2.0, 2.0, -8.0, -8.0, 0.0, math.nan, 1.0, 2.0, 10.0, 0.5, 1.0000000001, 7.0, math.inf, 1e-5])
    e = np.array([10.0, 0.5, 3.0, 1.0 / 3.0, 0.0, 0.0, math.nan, 1024.0, -3.0, 0.5, 1e9, -0.25, 2.0, 3.5])
    m = max(n - len(b), 0)
    b = np.concatenate([b, rng.random(m) * 100 + 0.01])[:n]
    e = np.concatenate([e, (rng.random(m) - 0.5) * 10])[:n]
    return b, e


def ulps(got, want):
    def key(a):  # IEEE totalOrder as integers: adjacent doubles differ by 1
        return [INT64_MIN - int(b) if b < 0 else int(b) for b in np.asarray(a, np.float64).view(np.int64)]
    return [abs(x - y) for x, y in zip(key(got), key(want))]


@pytest.mark.gpu
def test_power_against_math_pow(ctx):
    worst = 0
    for n in ROWS:
        b, e = power_inputs(n, 3 + n)
        vb, ve = null_mask(n, n + 5), null_mask(n, n + 6)
        for nulls in (False, True):
            cb = ctx.upload(b, vb if nulls else None, offset=3)
            ce = ctx.upload(e, ve if nulls else None)
            out = evaluate(ctx, [cb, ce], fn("Power", col(0), col(1)))
            assert out.dtype == F64 and len(out) == n
            keep = (vb & ve) if nulls else np.ones(n, bool)
            assert np.array_equal(validity(out), keep)
            got = out.to_numpy()[0][keep]
            want = np.array([ref_pow(float(x), float(y)) for x, y in zip(b, e)], np.float64)[keep]
            nan = np.isnan(want)
            assert np.array_equal(np.isnan(got), nan)
            d = ulps(got[~nan], want[~nan])
            worst = max([worst] + d)
    print("POWER: largest distance from math.pow = %d ULP" % worst)
    assert worst <= POWER_ULP_BOUND
    # a Float64 literal exponent broadcasts; an Int64 literal is the reference's type error
    b, _ = power_inputs(65, 1)
    out = evaluate(ctx, [ctx.upload(b)], fn("Power", col(0), lit(2.0)))
    want = np.array([ref_pow(float(x), 2.0) for x in b])
    nan = np.isnan(want)
    assert max(ulps(out.to_numpy()[0][~nan], want[~nan])) <= POWER_ULP_BOUND
    with pytest.raises(qe_hip.QehError) as err:
        evaluate(ctx, [ctx.upload(b)], fn("Power", col(0), lit(2)))
    assert err.value.status == abi.QEH_E_TYPE and err.value.message == "POWER requires float arguments"


# ---- GPU: strings ------------------------------------------------------------------------------------

def strings_of(col):
    return col.to_bytes()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["Upper", "Lower"])
def test_case_mapping_on_both_paths(ctx, name):
    ref = bytes.upper if name == "Upper" else bytes.lower
    for n in ROWS:
        slots = make_slots(n, 100 + n)
        want = [ref(s) for s in slots]
        # no NULLs: the stream path, over a slice at column offset 3 whose bytes start at an odd address
        c = sliced(ctx, slots)
        out, ran = launches(ctx, lambda: evaluate(ctx, [c], fn(name, col(0))), ["str_case_stream", "str_rows"])
        assert out.dtype == U8 and len(out) == n
        if sum(map(len, slots)):
            assert ran["str_case_stream"] == 1
        assert ran["str_rows"] == 0
        assert strings_of(out) == want, n
        assert out.c.null_count == 0 and validity(out).all()
        # NULL rows that own bytes: the row path; their result slots are empty
        valid = null_mask(n, 200 + n)
        c = sliced(ctx, slots, valid)
        out, ran = launches(ctx, lambda: evaluate(ctx, [c], fn(name, col(0))), ["str_case_stream", "str_rows"])
        assert ran == {"str_case_stream": 0, "str_rows": 1}
        assert np.array_equal(validity(out), valid)
        assert strings_of(out) == [w if v else b"" for w, v in zip(want, valid)], n


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["Upper", "Lower"])
def test_non_ascii_is_refused_in_valid_rows_only(ctx, name):
    slots = make_slots(70, 5)
    slots[40] = slots[40][:20] + "é".encode() + slots[40][22:]  # inside a whole 16-B line
    slots[3] = b"\xc3\xa9"                                        # and in the slice's unaligned head
    for bad_row in (40, 3):
        only = [s if i == bad_row else s.replace(b"\xc3\xa9", b"ee") for i, s in enumerate(slots)]
        with pytest.raises(qe_hip.QehError) as err:  # the stream path
            evaluate(ctx, [sliced(ctx, only)], fn(name, col(0)))
        assert err.value.status == abi.QEH_E_UNSUPPORTED
        assert name.upper() in err.value.message and "non-ASCII" in err.value.message
        valid = np.ones(70, bool)
        valid[7] = False
        with pytest.raises(qe_hip.QehError) as err:  # the row path: another row is NULL
            evaluate(ctx, [sliced(ctx, only, valid)], fn(name, col(0)))
        assert err.value.status == abi.QEH_E_UNSUPPORTED and "non-ASCII" in err.value.message
        valid[bad_row] = False  # the byte sits in a NULL row only: never inspected
        out = evaluate(ctx, [sliced(ctx, only, valid)], fn(name, col(0)))
        ref = bytes.upper if name == "Upper" else bytes.lower
        assert strings_of(out) == [ref(s) if v else b"" for s, v in zip(only, valid)]


@pytest.mark.gpu
def test_length_values_and_validity(ctx):
    for n in ROWS:
        slots = make_slots(n, 300 + n)
        for valid in (None, null_mask(n, 301 + n)):
            out, ran = launches(ctx, lambda: evaluate(ctx, [sliced(ctx, slots, valid)], fn("Length", col(0))), ["str_length"])
            assert out.dtype == I64 and len(out) == n and ran["str_length"] == (1 if n else 0)
            keep = np.ones(n, bool) if valid is None else valid
            assert np.array_equal(validity(out), keep)
            assert np.array_equal(out.to_numpy()[0][keep], np.array([len(s) for s in slots], np.int64)[keep])
    out = evaluate(ctx, [ctx.upload(np.arange(5))], fn("Length", lit("abc")))  # a literal broadcasts
    assert out.to_numpy()[0].tolist() == [3] * 5


@pytest.mark.gpu
def test_concat_reads_slots_whatever_their_validity(ctx):
    for n in ROWS:
        a, b, c = make_slots(n, 400 + n), make_slots(n, 401 + n)[::-1], make_slots(n, 402 + n)
        va = null_mask(n, 403 + n)
        ca, cb, cc = sliced(ctx, a, va), sliced(ctx, b), upload_slots(ctx, c, null_mask(n, 404 + n))
        cases = [
            (fn("Concat", col(0)), [a]),
            (fn("Concat", col(0), col(1)), [a, b]),
            (fn("Concat", col(0), lit(", "), col(2)), [a, b", ", c]),
            (fn("Concat", lit(""), col(1), lit("")), [b"", b, b""]),
            (fn("Concat", col(2), col(2), col(0)), [c, c, a]),
        ]
        for expr, parts in cases:
            out, ran = launches(ctx, lambda: evaluate(ctx, [ca, cb, cc], expr), ["str_rows", "str_case_stream"])
            assert out.dtype == U8 and len(out) == n
            assert ran == {"str_rows": 1, "str_case_stream": 0}
            assert (not out.c.validity) or out.c.null_count == 0
            assert validity(out).all()
            assert strings_of(out) == ref_concat(parts, n), n
    # more operands than one pass takes are folded
    cols = [upload_slots(ctx, make_slots(65, 500 + k)) for k in range(10)]
    out = evaluate(ctx, cols, fn("Concat", *[col(k) for k in range(10)]))
    assert strings_of(out) == ref_concat([make_slots(65, 500 + k) for k in range(10)], 65)
    out = evaluate(ctx, [cols[0]], fn("Concat", lit("ab"), lit("c")))  # literals only: n rows of them
    assert strings_of(out) == [b"abc"] * 65


@pytest.mark.gpu
def test_coalesce_is_its_first_argument(ctx):
    x = fill(I64_SPECIALS, 65, 1)
    va = null_mask(65, 2)
    a, b = ctx.upload(x, va), ctx.upload(np.arange(65))
    out = evaluate(ctx, [a, b], fn("Coalesce", col(0), col(1)))
    assert np.array_equal(validity(out), va) and np.array_equal(out.to_numpy()[0][va], x[va])
    out = evaluate(ctx, [a, b], fn("Coalesce", binop(col(1), BinaryOp.Add, lit(1)), col(0)))
    assert np.array_equal(out.to_numpy()[0], np.arange(65) + 1)
    with pytest.raises(qe_hip.QehError) as err:  # the ignored argument is still evaluated
        evaluate(ctx, [a, b], fn("Coalesce", col(1), binop(col(1), BinaryOp.Add, lit(INT64_MAX))))
    assert err.value.status == abi.QEH_E_OVERFLOW
    s = upload_slots(ctx, make_slots(65, 3), va)
    out = evaluate(ctx, [s, b], fn("Coalesce", col(0), col(1)))
    assert strings_of(out) == make_slots(65, 3) and np.array_equal(validity(out), va)


@pytest.mark.gpu
def test_unimplemented_functions_are_refused_after_their_arguments(ctx):
    a = ctx.upload(np.arange(10))
    with pytest.raises(qe_hip.QehError) as err:
        evaluate(ctx, [a], fn("Nullif", col(0), col(0)))
    assert err.value.status == abi.QEH_E_UNSUPPORTED and err.value.message == "Nullif function not yet fully implemented"
    with pytest.raises(qe_hip.QehError) as err:
        evaluate(ctx, [a], fn("Nullif", binop(col(0), BinaryOp.Divide, lit(0)), col(0)))
    assert err.value.status == abi.QEH_E_DIV0
    with pytest.raises(qe_hip.QehError) as err:
        evaluate(ctx, [upload_slots(ctx, [b"a b"] * 10)], fn("ToTsQuery", col(0)))
    assert err.value.status == abi.QEH_E_UNSUPPORTED and "TO_TSQUERY" in err.value.message
    with pytest.raises(qe_hip.QehError) as err:
        evaluate(ctx, [a], fn("Ceil", col(0)))
    assert err.value.status == abi.QEH_E_TYPE and err.value.message == "CEIL requires float argument"
    with pytest.raises(qe_hip.QehError) as err:
        evaluate(ctx, [a], fn("Upper"))
    assert err.value.status == abi.QEH_E_INVALID and err.value.message == "UPPER requires 1 argument"


# ---- GPU: composition --------------------------------------------------------------------------------

@pytest.mark.gpu
def test_functions_compose_with_arithmetic(ctx):
    for n in ROWS:
        rng = np.random.default_rng(n)
        p, q = rng.integers(-10 ** 9, 10 ** 9, n), rng.integers(-10 ** 9, 10 ** 9, n)
        vp = null_mask(n, n + 9)
        out = evaluate(ctx, [ctx.upload(p, vp), ctx.upload(q)], fn("Abs", binop(col(0), BinaryOp.Subtract, col(1))), n)
        assert np.array_equal(validity(out), vp) and np.array_equal(out.to_numpy()[0][vp], np.abs(p - q)[vp])
        x = fill(F64_SPECIALS, n, n)
        out = evaluate(ctx, [ctx.upload(x)], fn("Sqrt", binop(col(0), BinaryOp.Multiply, col(0))), n)
        assert same_bits(out.to_numpy()[0], [ref_sqrt(float(v) * float(v)) for v in x])
        # the function's result feeds the interpreter again
        out = evaluate(ctx, [ctx.upload(p), ctx.upload(q)],
                       binop(fn("Abs", binop(col(0), BinaryOp.Subtract, col(1))), BinaryOp.Add, lit(1)), n)
        assert np.array_equal(out.to_numpy()[0], np.abs(p - q) + 1)
    with pytest.raises(qe_hip.QehError) as err:  # the argument's own error wins
        evaluate(ctx, [ctx.upload(np.array([1, 2, 3]))], fn("Abs", binop(col(0), BinaryOp.Add, lit(INT64_MAX))))
    assert err.value.status == abi.QEH_E_OVERFLOW


@pytest.mark.gpu
def test_upper_equals_literal_through_filter_and_filter_limit(ctx):
    names = [b"Bob", b"bob", b"BOB", b"bo", b"Bobb", b"", b"alice", b"bOb"] * 40
    valid = np.ones(len(names), bool)
    valid[2::16] = False  # some BOBs are NULL: dropped
    ids = np.arange(len(names))
    pred = binop(fn("Upper", col(0)), BinaryOp.Equal, lit("BOB"))
    want = np.array([i for i, (s, v) in enumerate(zip(names, valid)) if v and s.upper() == b"BOB"])
    for cname in (upload_slots(ctx, names, valid), sliced(ctx, names)):
        w = want if cname.c.validity else np.array([i for i, s in enumerate(names) if s.upper() == b"BOB"])
        (out, rows), ran = launches(ctx, lambda: ctx.filter([cname, ctx.upload(ids)], pred, out_idx=[1]), ["utf8_compare"])
        assert ran["utf8_compare"] == 1  # column-against-literal on the existing kernel
        assert rows == len(w) and np.array_equal(out[0].to_numpy()[0], w)
        out, rows = ctx.filter([cname, ctx.upload(ids)], pred, out_idx=[1, 0], max_rows=7)
        assert rows == 7 and np.array_equal(out[0].to_numpy()[0], w[:7])
        assert [s.upper() for s in out[1].to_bytes()] == [b"BOB"] * 7
    a, b = make_slots(257, 1), make_slots(257, 2)[::-1]
    pred = binop(fn("Length", fn("Concat", col(0), col(1))), BinaryOp.Greater, lit(3))
    out, rows = ctx.filter([upload_slots(ctx, a), upload_slots(ctx, b), ctx.upload(np.arange(257))], pred, out_idx=[2])
    want = [i for i in range(257) if len(a[i]) + len(b[i]) > 3]
    assert rows == len(want) and out[0].to_numpy()[0].tolist() == want


@pytest.mark.gpu
def test_fused_entry_points_refuse_a_function_by_name(ctx):
    k, v = ctx.upload(np.arange(100) % 7), ctx.upload(np.arange(100, dtype=np.float64))
    pred = binop(fn("Abs", col(1)), BinaryOp.Greater, lit(3.0))
    with pytest.raises(qe_hip.QehError) as err:
        ctx.filter_aggregate([k, v], pred, [0], [qe_hip.agg(AF.Sum, 1)])
    assert err.value.status == abi.QEH_E_UNSUPPORTED and "QEH_EX_SCALAR_FUNCTION" in err.value.message


# ---- GPU: plans over employees x departments ------------------------------------------------------------

ID, NAME, AGE, SALARY, DEPT, SALARY_F = range(6)
D_ID, D_NAME = 6, 7  # departments' columns after a join with the six employee columns


@pytest.fixture(scope="module")
def srcs():
    import pyarrow as pa
    import pyarrow.csv as pacsv
    emp = pacsv.read_csv(os.path.join(GOLD, "employees.csv"))  # "NULL" is read as a NULL
    dep = pacsv.read_csv(os.path.join(GOLD, "departments.csv"))
    assert emp["dept_id"].null_count == 1 and str(emp["salary"].type) == "int64"
    emp = emp.append_column("salary_f", emp["salary"].cast(pa.float64()))
    return (MemoryDataSource(emp.schema, emp.to_batches()), MemoryDataSource(dep.schema, dep.to_batches()))


def column(batches, i=0):
    return [v for b in batches for v in b.column(i).to_pylist()]


SALARIES = [75000, 85000, 95000, 80000, 90000, 78000]
NAMES = ["Alice", "Bob", "Charlie", "Diana", "Eve", "Frank"]


@pytest.mark.gpu
def test_plan_projection_of_functions(ctx, srcs):
    emp, _ = srcs
    plan = Projection(Scan(emp), [fn("Upper", col(NAME)), fn("Length", col(NAME)),
                                  fn("Round", binop(col(SALARY_F), BinaryOp.Divide, lit(7.0)))], ["u", "l", "r"])
    (b,) = QueryExecutor(ctx).execute(plan)
    assert [str(f.type) for f in b.schema] == ["string", "int64", "double"]
    assert b.column(0).to_pylist() == [s.upper() for s in NAMES]
    assert b.column(1).to_pylist() == [len(s) for s in NAMES]
    assert b.column(2).to_pylist() == [ref_round(s / 7.0) for s in SALARIES]


@pytest.mark.gpu
def test_plan_filter_and_sort_by_functions(ctx, srcs, monkeypatch):
    emp, _ = srcs
    ex = QueryExecutor(ctx)
    lower = binop(fn("Lower", col(NAME)), BinaryOp.Equal, lit("alice"))
    assert column(ex.execute(Filter(Scan(emp), lower)), NAME) == ["Alice"]
    by_len = Sort(Scan(emp), [fn("Length", col(NAME))], [True])  # stable: ties keep the input order
    assert column(ex.execute(by_len), NAME) == ["Bob", "Eve", "Alice", "Diana", "Frank", "Charlie"]
    # Projection(Filter) and Limit(Filter), Limit(Sort): the fusions rewrite first or step aside
    long_names = Projection(Filter(Scan(emp), binop(fn("Length", col(NAME)), BinaryOp.Greater, lit(3))),
                            [fn("Upper", col(NAME))], ["u"])
    top2 = Limit(by_len, 0, 2)
    for no_fusion in (False, True):
        if no_fusion:
            monkeypatch.setenv("QEH_NO_FUSION", "1")
        assert column(ex.execute(long_names)) == ["ALICE", "CHARLIE", "DIANA", "FRANK"]
        assert column(ex.execute(Limit(long_names, 1, 2))) == ["CHARLIE", "DIANA"]
        assert column(ex.execute(Limit(Filter(Scan(emp), lower), 0, 1)), NAME) == ["Alice"]
        assert column(ex.execute(top2), NAME) == ["Bob", "Eve"]


@pytest.mark.gpu
@pytest.mark.parametrize("no_fusion", [False, True], ids=["fused", "no_fusion"])
def test_plan_coalesce_of_a_column_outlives_its_input(ctx, srcs, monkeypatch, no_fusion):
    """COALESCE(column, ..) is a view of the operator's input: it has to keep that input's buffers
    alive after the Projection returns and the filtered table is dropped.  The operators above it
    allocate (same size classes), so a column left dangling would be overwritten."""
    emp, _ = srcs
    if no_fusion:
        monkeypatch.setenv("QEH_NO_FUSION", "1")
    ex = QueryExecutor(ctx)
    older = Filter(Scan(emp), binop(col(AGE), BinaryOp.Greater, lit(26)))  # Bob Charlie Diana Eve Frank
    inner = Projection(older, [fn("Coalesce", col(NAME), lit("x")), fn("Coalesce", col(SALARY), col(AGE)),
                               fn("Coalesce", fn("Coalesce", col(DEPT), col(ID)), col(ID))], ["n", "s", "d"])
    outer = Projection(inner, [col(0), col(1), col(2), fn("Upper", col(0)), binop(col(1), BinaryOp.Add, lit(1)),
                               fn("Length", col(0)), fn("Concat", col(0), lit("-"), col(0))],
                       ["n", "s", "d", "u", "s1", "l", "nn"])
    names, pay = NAMES[1:], SALARIES[1:]
    (b,) = ex.execute(outer)
    assert [str(f.type) for f in b.schema] == ["string", "int64", "int64", "string", "int64", "int64", "string"]
    assert b.column(0).to_pylist() == names and b.column(1).to_pylist() == pay
    assert b.column(2).to_pylist() == [102, 101, 103, 102, None]
    assert b.column(3).to_pylist() == [s.upper() for s in names]
    assert b.column(4).to_pylist() == [s + 1 for s in pay]
    assert b.column(5).to_pylist() == [len(s) for s in names]
    assert b.column(6).to_pylist() == [s + "-" + s for s in names]
    (b,) = ex.execute(Sort(inner, [col(1)], [True]))
    assert b.column(0).to_pylist() == ["Frank", "Diana", "Bob", "Eve", "Charlie"]
    assert b.column(1).to_pylist() == sorted(pay) and b.column(2).to_pylist() == [None, 103, 102, 102, 101]
    (b,) = ex.execute(inner)  # the Projection as the root: its columns are exported after `older` is gone
    assert b.column(0).to_pylist() == names and b.column(1).to_pylist() == pay


@pytest.mark.gpu
def test_plan_window_keys_and_arguments_take_functions(ctx, srcs):
    from qe_hip import Window, WindowExpr, WindowFunctionType as W
    emp, _ = srcs
    away = fn("Abs", binop(col(SALARY), BinaryOp.Subtract, lit(85000)))  # 10000 0 10000 5000 5000 7000
    plan = Window(Scan(emp), [WindowExpr(W.RowNumber, [], [fn("Length", col(NAME))], [away]),
                              WindowExpr(W.Lag, [fn("Length", col(NAME))], [], [col(ID)])],
                  ["id", "name", "age", "salary", "dept_id", "salary_f", "rn", "prev_len"])
    (b,) = QueryExecutor(ctx).execute(plan)
    # by name length: {Bob 0, Eve 5000}, {Diana 5000, Frank 7000, Alice 10000}, {Charlie}
    assert b.column(6).to_pylist() == [3, 1, 1, 1, 2, 2]
    assert b.column(7).to_pylist() == [None, 5, 3, 7, 5, 3]


def joined(emp, dep):
    return HashJoin(Scan(emp), Scan(dep), JoinType.Inner, binop(col(DEPT), BinaryOp.Equal, col(D_ID)))


@pytest.mark.gpu
@pytest.mark.parametrize("no_fusion", [False, True], ids=["fused", "no_fusion"])
def test_plan_functions_around_joins_and_aggregates(ctx, srcs, monkeypatch, no_fusion):
    emp, dep = srcs
    if no_fusion:
        monkeypatch.setenv("QEH_NO_FUSION", "1")
    ex = QueryExecutor(ctx)
    # GROUP BY UPPER(dept_name), SUM(ABS(salary - 85000)): Engineering 10000 + 10000, Sales 0 + 5000, HR 5000
    plan = HashAggregate(joined(emp, dep), [fn("Upper", col(D_NAME))],
                         [AggregateExpr(AF.Sum, fn("Abs", binop(col(SALARY), BinaryOp.Subtract, lit(85000))))])
    (b,) = ex.execute(plan)
    assert sorted(zip(column([b], 0), column([b], 1))) == [("ENGINEERING", 20000), ("HR", 5000), ("SALES", 5000)]
    # Filter(HashJoin) with a function over the build side's strings
    plan = Filter(joined(emp, dep), binop(fn("Upper", col(D_NAME)), BinaryOp.Equal, lit("SALES")))
    assert sorted(column(ex.execute(plan), NAME)) == ["Bob", "Eve"]
    # HashAggregate(Filter(X)): the fused filter-aggregate steps aside for a function predicate
    plan = HashAggregate(Filter(Scan(emp), binop(fn("Length", col(NAME)), BinaryOp.Greater, lit(3))), [col(DEPT)],
                         [AggregateExpr(AF.Sum, col(SALARY))])
    (b,) = ex.execute(plan)
    got = sorted(zip(column([b], 0), column([b], 1)), key=lambda r: (r[0] is None, r[0]))
    assert got == [(101, 170000), (103, 80000), (None, 78000)]
    # HashAggregate(Filter(HashJoin)), the fused join-aggregate's shape, with a function in the predicate:
    # |salary - 85000| >= 5000 keeps Alice, Charlie (Engineering), Diana (HR), Eve (Sales)
    pred = binop(fn("Abs", binop(col(SALARY_F), BinaryOp.Subtract, lit(85000.0))), BinaryOp.GreaterEqual, lit(5000.0))
    plan = HashAggregate(Filter(joined(emp, dep), pred), [col(D_NAME)], [AggregateExpr(AF.Sum, col(SALARY))])
    (b,) = ex.execute(plan)
    assert sorted(zip(column([b], 0), column([b], 1))) == [("Engineering", 170000), ("HR", 80000), ("Sales", 90000)]
    # a join condition with a function conjunct: dept ids match and the department's name is short
    on = binop(col(DEPT), BinaryOp.Equal, col(D_ID)) & binop(fn("Length", col(D_NAME)), BinaryOp.Less, lit(6))
    plan = HashJoin(Scan(emp), Scan(dep), JoinType.Inner, on)
    assert sorted(column(ex.execute(plan), NAME)) == ["Bob", "Diana", "Eve"]
