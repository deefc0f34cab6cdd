"""Expression programs at the edges of their domain: the device interpreter (run_program, csrc/expr_device.h)
and the CPU oracle (oracle/qe_oracle.c) against the exact model of the reference in expr_model.py.

CPU tests (oracle against model): the integer edge grid under + - * / % and unary minus, the coercing
compares around 2^53 and 2^63, the AND / OR / NOT truth tables, 300 seeded random trees, and the
first-error cases.  GPU tests (device against model): the same grid laid out over two tiles plus 17
rows of each kernel that carries the interpreter, the random trees, the first-error cases at all four
call sites, and the program limits (8 value slots, 40 instructions).

Which error wins: evaluate_expr is post-order and every operator finishes its whole array, rows in
order and NULL rows skipped, before the next one starts; so the error reported is the one with the
least (post-order node, row) among the valid rows that raise."""
import functools
import os
import re

import numpy as np
import pytest

import expr_model as em
import oracle_bind as ob
import sliced
from qe_hip import AggregateFunction as AF
from qe_hip import BinaryOp, QehError, ScalarValue, UnaryExpr, UnaryOp, abi, binop, col, lit
from qe_hip.expr import Literal

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "query-engine_amd", "csrc")


def _const(src, name):
    with open(os.path.join(CSRC, src)) as f:
        return int(re.search(r"constexpr int %s = (\d+);" % name, f.read()).group(1))


K_BLOCK, K_FR, K_ER, K_AGGR = (_const("device_common.h", "kBlock"), _const("k_filter.hip", "kFR"),
                               _const("k_filter.hip", "kER"), _const("agg_device.h", "kAggR"))
K_NS, K_MAX_INSTR = _const("expr.h", "kNS"), _const("expr.h", "kMaxInstr")


class Site:
    """A kernel that calls run_program: a lane holds `rows` rows `stride` apart; `tile` rows per
    workgroup step.  Every test size is two tiles plus 17 rows."""

    def __init__(self, rows, stride, tile):
        self.rows, self.stride, self.tile, self.n = rows, stride, tile, 2 * tile + 17


SITES = {
    "k_eval": Site(K_ER, 64, K_BLOCK * K_ER),
    "k_filter": Site(K_FR, K_BLOCK, K_BLOCK * K_FR),
    "k_agg_rows": Site(K_AGGR, 64, K_BLOCK * K_AGGR),
    "k_groupby_lds": Site(K_AGGR, 64, K_BLOCK * K_AGGR),
}
# how an expression reaches each kernel; a predicate form wraps the expression in a compare
FORMS = {
    "k_eval": ["eval"],
    "k_filter": ["filter", "filter_limit10"],
    "k_agg_rows": ["agg_no_key", "agg_key_table"],   # GM_ZERO; GM_GROUP (QEH_NO_LDS_GROUPBY)
    "k_groupby_lds": ["agg_key_lds"],
}
SITE_FORMS = [(s, f) for s in SITES for f in FORMS[s]]
N_KEYS = 5

INT_T = {"int64": em.INT64, "int32": em.INT32}
NP_T = {em.INT64: np.int64, em.INT32: np.int32, em.FLOAT64: np.float64, em.FLOAT32: np.float32, em.BOOL: np.bool_}
OPS = {"add": BinaryOp.Add, "sub": BinaryOp.Subtract, "mul": BinaryOp.Multiply, "div": BinaryOp.Divide,
       "mod": BinaryOp.Modulo}
CMPS = {"eq": BinaryOp.Equal, "ne": BinaryOp.NotEqual, "lt": BinaryOp.Less, "le": BinaryOp.LessEqual,
        "gt": BinaryOp.Greater, "ge": BinaryOp.GreaterEqual}


def edge_values(t):
    bits = em.BITS[t]
    lo, hi = em.RANGE[t]
    vals = [lo, lo + 1, lo + 2, hi, hi - 1, hi - 2, 0, 1, -1, 2, -2, 3, -3, 7, -7,
            lo // 2, lo // 2 - 1, hi // 2, hi // 2 + 1,
            2 ** ((bits - 1) // 2), -2 ** ((bits - 1) // 2), 2 ** (bits // 2),
            3037000499, -3037000499, 3037000500, -3037000500, 46340, -46340, 46341, -46341]
    return [v for v in dict.fromkeys(vals) if lo <= v <= hi]


def typed_lit(t, v):
    return Literal({em.INT64: ScalarValue.Int64, em.INT32: ScalarValue.Int32, em.FLOAT64: ScalarValue.Float64,
                    em.FLOAT32: ScalarValue.Float32, em.BOOL: ScalarValue.Boolean}[t](v))


def outcome(fn):
    """('error', status, message) or ('ok', payload) of one run, whichever backend ran it."""
    try:
        return ("ok", fn())
    except (em.ModelError, ob.OracleError, QehError) as e:
        return ("error", e.status, e.message)


def bits_of(v):
    v = np.asarray(v)
    return v.view({4: np.int32, 8: np.int64}[v.dtype.itemsize]) if v.dtype.kind == "f" else v


def canon(values, valid, dtype=None):
    """A column as (dtype, validity, value bits with NULL rows zeroed): equal iff the columns are."""
    values = np.asarray(values)
    valid = np.ones(len(values), bool) if valid is None else np.asarray(valid, bool)
    if dtype is not None:
        values = values.astype(NP_T[dtype])
    return (values.dtype.name, valid.tolist(), np.where(valid, bits_of(values), 0).tolist())


def assert_same(got, want, what):
    if got == want:
        return
    if "error" in (got[0], want[0]):
        brief = lambda o: o if o[0] == "error" else "a result"  # noqa: E731
        raise AssertionError("%s: got %r, expected %r" % (what, brief(got), brief(want)))
    raise AssertionError("%s: results differ: %s" % (what, first_difference(got[1], want[1])))


def first_difference(g, w, path=""):
    if type(g) is not type(w):
        return "%s: %r vs %r" % (path, g, w)
    if isinstance(g, (list, tuple)):
        if len(g) != len(w):
            return "%s: length %d vs %d" % (path, len(g), len(w))
        for i, (a, b) in enumerate(zip(g, w)):
            if a != b:
                return first_difference(a, b, "%s[%d]" % (path, i))
    if isinstance(g, dict):
        return "%s: %r vs %r" % (path, sorted(g.items())[:8], sorted(w.items())[:8])
    return "%s: %r vs %r" % (path, g, w)


# ---- one expression through one form, by each backend ----------------------------------------------
# cols: (values, validity-or-None) pairs.  A predicate form appends a non-null Int64 key column and
# counts column 0.  Payloads are plain Python values that compare exactly.

def predicate_of(expr):
    return binop(expr, BinaryOp.Greater, lit(0))


def key_column(n):
    return (np.arange(n, dtype=np.int64) * 7 + 3) % N_KEYS, None


def selection_payload(form, cols, sel):
    """What a predicate form returns for the rows `sel` (bool mask) of `cols`."""
    n = len(sel)
    if form.startswith("filter"):
        rows = np.flatnonzero(sel)
        if form == "filter_limit10":
            rows = rows[:10]
        return (len(rows), [canon(np.asarray(v)[rows], None if m is None else np.asarray(m)[rows]) for v, m in cols])
    counted = sel & (np.ones(n, bool) if cols[0][1] is None else np.asarray(cols[0][1], bool))
    if form == "agg_no_key":
        return int(counted.sum())
    key = key_column(n)[0]
    return {int(k): int((counted & (key == k)).sum()) for k in np.unique(key[sel])}


def model_run(form, cols, expr):
    def run():
        if form == "eval":
            r = em.evaluate_expr(expr, cols)
            return canon(*r.to_numpy())
        r = em.evaluate_expr(predicate_of(expr), cols)
        assert r.dtype == em.BOOL
        v, m = r.to_numpy()
        return selection_payload(form, cols, v & m)
    return outcome(run)


def oracle_run(form, cols, expr):
    hc = [ob.HostCol(v, m) for v, m in cols]
    n = len(cols[0][0])

    def run():
        if form == "eval":
            (v, m), dt = ob.eval_expr(hc, expr, n)
            return canon(v, m, dt)
        rows, _, _ = ob.filter(hc + [ob.HostCol(np.arange(n, dtype=np.int64))], predicate_of(expr), out_idx=[len(hc)])
        sel = np.zeros(n, bool)
        sel[rows[0][0]] = True
        return selection_payload(form, cols, sel)
    return outcome(run)


def upload(ctx, cols, slice_poison=None):
    """slice_poison: upload every column inside a poisoned parent at Arrow offset 3 (sliced.make);
    slice_poison[j] gives column j's poison values, None the type's default poison."""
    if slice_poison is None:
        return [ctx.upload(v, m) for v, m in cols]
    return [sliced.make(v, m, lead=3, poison=slice_poison.get(j)).dev(ctx) for j, (v, m) in enumerate(cols)]


def device_run(ctx, monkeypatch, form, cols, expr, slice_poison=None):
    n = len(cols[0][0])

    def run():
        dev = upload(ctx, cols, slice_poison)
        if form == "eval":
            out = ctx.eval(dev, expr)
            return canon(*out.to_numpy(), dtype=out.dtype)
        pred = predicate_of(expr)
        if form.startswith("filter"):
            out, rows = ctx.filter(dev, pred, max_rows=10 if form == "filter_limit10" else None)
            return (rows, [canon(*c.to_numpy()) for c in out])
        dev.append(ctx.upload(*key_column(n)))
        if form == "agg_key_table":
            monkeypatch.setenv("QEH_NO_LDS_GROUPBY", "1")
        else:
            monkeypatch.delenv("QEH_NO_LDS_GROUPBY", raising=False)
        gk, ga, g = ctx.filter_aggregate(dev, pred, [] if form == "agg_no_key" else [len(cols)], [(AF.Count, 0)])
        if g == 0:
            return 0 if form == "agg_no_key" else {}
        (cnt, cm), = [c.to_numpy() for c in ga]
        assert cm is None or cm.all()
        if form == "agg_no_key":
            assert g == 1
            return int(cnt[0])
        (k, km), = [c.to_numpy() for c in gk]
        assert km is None or km.all()
        assert len(set(k.tolist())) == len(k) == g
        return {int(a): int(b) for a, b in zip(k, cnt)}
    return outcome(run)


# ---- the integer edge grid ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def grid(tname):
    """(a, b): every ordered pair of the type's edge values, as two columns."""
    e = edge_values(INT_T[tname])
    dt = NP_T[INT_T[tname]]
    return np.repeat(np.array(e, dt), len(e)), np.tile(np.array(e, dt), len(e))


@functools.lru_cache(maxsize=None)
def grid_cells(tname, opname):
    """The model's outcome of every cell on its own: ('ok', canon) or ('error', status, message)."""
    a, b = grid(tname)
    expr = binop(col(0), OPS[opname], col(1))
    return [model_run("eval", [(a[i:i + 1], None), (b[i:i + 1], None)], expr) for i in range(len(a))]


def test_edge_values_hold_what_the_issue_lists():
    e64, e32 = edge_values(em.INT64), edge_values(em.INT32)
    assert len(e64) == 30 and len(e32) == 26 and len(set(e64)) == 30 and len(set(e32)) == 26
    for v in (-2 ** 63, 2 ** 63 - 1, -2 ** 62 - 1, 2 ** 62, 2 ** 31, -2 ** 31, 2 ** 32, 3037000500, -3037000499):
        assert v in e64
    for v in (-2 ** 31, 2 ** 31 - 1, -2 ** 30 - 1, 2 ** 30, 2 ** 15, -2 ** 15, 2 ** 16, 46341, -46340):
        assert v in e32


@pytest.mark.parametrize("opname", sorted(OPS))
@pytest.mark.parametrize("tname", sorted(INT_T))
def test_oracle_edge_grid(tname, opname):
    """Every ordered pair: the cells the model raises on raise the same status and message in the
    oracle, one by one; the others agree in value, validity and dtype in one call."""
    a, b = grid(tname)
    cells = grid_cells(tname, opname)
    expr = binop(col(0), OPS[opname], col(1))
    bad = np.array([c[0] == "error" for c in cells])
    assert bad.any() and not bad.all()
    for i in np.flatnonzero(bad):
        cols = [(a[i:i + 1], None), (b[i:i + 1], None)]
        assert_same(oracle_run("eval", cols, expr), cells[i], "%d %s %d" % (a[i], opname, b[i]))
    cols = [(a[~bad], None), (b[~bad], None)]
    want = model_run("eval", cols, expr)
    assert want[0] == "ok"
    assert_same(oracle_run("eval", cols, expr), want, "%s %s, the cells that do not raise" % (tname, opname))


@pytest.mark.parametrize("tname", sorted(INT_T))
def test_oracle_unary_minus_wraps(tname):
    t = INT_T[tname]
    e = np.array(edge_values(t), NP_T[t])
    cols = [(e, None)]
    want = model_run("eval", cols, UnaryExpr(UnaryOp.Minus, col(0)))
    assert want[0] == "ok" and want[1][2][0] == em.RANGE[t][0]  # -MIN == MIN
    assert_same(oracle_run("eval", cols, UnaryExpr(UnaryOp.Minus, col(0))), want, tname)


def masked_grid(tname, opname, n):
    """The grid repeated to n rows; a cell that raises is NULL in one operand (left and right in turn),
    so nothing raises and the launch also shows that a NULL row never does."""
    a, b = grid(tname)
    bad = np.array([c[0] == "error" for c in grid_cells(tname, opname)])
    idx = np.arange(n) % len(a)
    left = (np.arange(len(a)) % 2 == 0)
    return [(a[idx], ~(bad & left)[idx]), (b[idx], ~(bad & ~left)[idx])]


@functools.lru_cache(maxsize=None)
def masked_grid_model(tname, opname, site, form):
    cols = masked_grid(tname, opname, SITES[site].n)
    want = model_run(form, cols, binop(col(0), OPS[opname], col(1)))
    assert want[0] == "ok", want
    return cols, want


@pytest.mark.gpu
@pytest.mark.parametrize("opname", sorted(OPS))
@pytest.mark.parametrize("tname", sorted(INT_T))
@pytest.mark.parametrize("site,form", SITE_FORMS)
def test_device_edge_grid(ctx, monkeypatch, site, form, tname, opname):
    cols, want = masked_grid_model(tname, opname, site, form)
    got = device_run(ctx, monkeypatch, form, cols, binop(col(0), OPS[opname], col(1)))
    assert_same(got, want, "%s %s %s %s" % (site, form, tname, opname))


@pytest.mark.gpu
@pytest.mark.parametrize("tname", sorted(INT_T))
def test_device_unary_minus_wraps(ctx, monkeypatch, tname):
    t = INT_T[tname]
    e = np.array(edge_values(t), NP_T[t])
    cols = [(e[np.arange(SITES["k_eval"].n) % len(e)], None)]
    expr = UnaryExpr(UnaryOp.Minus, col(0))
    assert_same(device_run(ctx, monkeypatch, "eval", cols, expr), model_run("eval", cols, expr), tname)


# ---- coercing compares -------------------------------------------------------------------------------

def coercion_cases():
    """name -> (left column, right column): every left value against every right value."""
    i64 = [2 ** 53 - 1, 2 ** 53, 2 ** 53 + 1, 2 ** 62 + 1, 2 ** 63 - 1, -2 ** 63, -(2 ** 53) - 1, 0]
    f64 = [2.0 ** 53, 2.0 ** 53 + 2, 2.0 ** 63, -2.0 ** 63, 0.0, -0.0]
    i32 = [2 ** 31 - 1, -2 ** 31, 16777217, 0, -1]
    f64_for_i32 = [2147483647.0, 2147483647.5, -2147483648.0, 16777217.0, 16777216.0, -0.0, -1.0]
    f32 = np.array([0.1, 16777216.0, 1.0, -0.0, 3.4028235e38], np.float32)
    f64_for_f32 = [0.1, float(np.float32(0.1)), 16777217.0, 16777216.0, 1.0 + 2.0 ** -40, 0.0, 3.4028235e38]
    i64_for_i32 = [2 ** 31 - 1, 2 ** 31, -2 ** 31, -2 ** 31 - 1, 2 ** 32 - 1, 0, -1]

    def cross(l, lt, r, rt):
        l, r = np.asarray(l, lt), np.asarray(r, rt)
        return np.repeat(l, len(r)), np.tile(r, len(l))
    return {
        "int64_float64": cross(i64, np.int64, f64, np.float64),
        "float64_int64": cross(f64, np.float64, i64, np.int64),
        "int32_float64": cross(i32, np.int32, f64_for_i32, np.float64),
        "float32_float64": cross(f32, np.float32, f64_for_f32, np.float64),
        "float64_float32": cross(f64_for_f32, np.float64, f32, np.float32),
        "int32_int64": cross(i32, np.int32, i64_for_i32, np.int64),
        "int64_int32": cross(i64_for_i32, np.int64, i32, np.int32),
        "int32_float32": cross(i32, np.int32, f32, np.float32),
    }


COERCIONS = coercion_cases()


def coercion_exprs(name, cmp):
    """column against column, and column against each distinct right value as a literal (Float64 and
    Int64 literals only: what the planner types)."""
    l, r = COERCIONS[name]
    out = [("column", binop(col(0), CMPS[cmp], col(1)))]
    if r.dtype in (np.float64, np.int64):
        for v in dict.fromkeys(r.tolist()):
            out.append(("literal %r" % v, binop(col(0), CMPS[cmp], lit(v))))
    return out


@pytest.mark.parametrize("cmp", sorted(CMPS))
@pytest.mark.parametrize("name", sorted(COERCIONS))
def test_oracle_coercing_compares(name, cmp):
    l, r = COERCIONS[name]
    valid = np.arange(len(l)) % 11 != 5
    cols = [(l, valid), (r, None)]
    for what, expr in coercion_exprs(name, cmp):
        want = model_run("eval", cols, expr)
        assert want[0] == "ok" and want[1][0] == "bool"
        assert_same(oracle_run("eval", cols, expr), want, "%s %s %s" % (name, cmp, what))


def test_model_rounds_int64_to_float64_as_the_reference_casts():
    """2^53 + 1 rounds to 2^53 (ties to even), 2^63 - 1 to 2^63: `x as f64` (operators.rs:630)."""
    cols = [(np.array([2 ** 53 + 1, 2 ** 63 - 1, 2 ** 53 - 1], np.int64), None)]
    for v, want in ((2.0 ** 53, [True, False, False]), (2.0 ** 63, [False, True, False])):
        got, _ = em.evaluate_expr(binop(col(0), BinaryOp.Equal, lit(v)), cols).to_numpy()
        assert got.tolist() == want


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(COERCIONS))
def test_device_coercing_compares(ctx, monkeypatch, name):
    """All six operators, columns and literals, laid over two k_eval tiles plus 17 rows."""
    l, r = COERCIONS[name]
    idx = np.arange(SITES["k_eval"].n) % len(l)
    cols = [(l[idx], idx % 11 != 5), (r[idx], None)]
    for cmp in sorted(CMPS):
        for what, expr in coercion_exprs(name, cmp):
            assert_same(device_run(ctx, monkeypatch, "eval", cols, expr), model_run("eval", cols, expr),
                        "%s %s %s" % (name, cmp, what))


# ---- type errors -------------------------------------------------------------------------------------

TYPE_ERRORS = {  # columns: 0 Int64, 1 Int32, 2 Float64, 3 Boolean
    "no_coercion_in_arithmetic": (binop(col(0), BinaryOp.Multiply, lit(1.5)), "Unsupported types for multiplication"),
    "int64_plus_int32": (binop(col(0), BinaryOp.Add, col(1)), "Unsupported types for addition"),
    "modulo_of_floats": (binop(col(2), BinaryOp.Modulo, col(2)), "Modulo operation requires integer arrays"),
    "compare_with_null": (binop(col(0), BinaryOp.Greater, lit(None)),
                          "Invalid argument error: Invalid comparison operation: Int64 > Null"),
    "compare_bool_with_int": (binop(col(3), BinaryOp.Equal, col(0)),
                              "Invalid argument error: Invalid comparison operation: Boolean == Int64"),
    "and_of_ints": (col(0) & col(3), "AND requires boolean arrays"),
    "not_of_int": (UnaryExpr(UnaryOp.Not, col(0)), "NOT operator requires boolean array"),
    "minus_of_bool": (UnaryExpr(UnaryOp.Minus, col(3)), "Unsupported type for negation"),
}


@pytest.mark.parametrize("name", sorted(TYPE_ERRORS))
def test_oracle_type_errors(name):
    expr, message = TYPE_ERRORS[name]
    cols = [(np.arange(5, dtype=np.int64), None), (np.arange(5, dtype=np.int32), None), (np.arange(5) / 2, None),
            (np.arange(5) % 2 == 0, None)]
    want = model_run("eval", cols, expr)
    assert want == ("error", abi.QEH_E_TYPE, message)
    assert_same(oracle_run("eval", cols, expr), want, name)


def test_oracle_value_error_of_an_earlier_node_comes_before_a_type_error():
    """(a / 0) * 1.5: the reference divides before it looks at the multiplication's types."""
    cols = [(np.arange(5, dtype=np.int64), None)]
    expr = binop(binop(col(0), BinaryOp.Divide, lit(0)), BinaryOp.Multiply, lit(1.5))
    want = model_run("eval", cols, expr)
    assert want == ("error", abi.QEH_E_DIV0, em.MSG_DIV0)
    assert_same(oracle_run("eval", cols, expr), want, "(a / 0) * 1.5")


# ---- truth tables ------------------------------------------------------------------------------------

def truth_table_columns():
    tri = [(1, True), (0, True), (0, False), (1, False)]  # TRUE, FALSE, NULL over either payload
    a = [x for x in tri for _ in tri]
    b = [y for _ in tri for y in tri]
    return [(np.array([v for v, _ in c], bool), np.array([m for _, m in c], bool)) for c in (a, b)]


LOGIC = {"and": col(0) & col(1), "or": col(0) | col(1), "not": UnaryExpr(UnaryOp.Not, col(0))}


@pytest.mark.parametrize("name", sorted(LOGIC))
def test_oracle_truth_tables(name):
    cols = truth_table_columns()
    want = model_run("eval", cols, LOGIC[name])
    v, m = np.array(want[1][2], bool), np.array(want[1][1])
    a, am = cols[0]
    b, bm = cols[1]
    if name == "not":
        assert (m == am).all() and (v[m] == ~a[m]).all()
    else:  # non-Kleene: NULL if either side is NULL, FALSE AND NULL included
        assert (m == (am & bm)).all() and (v[m] == ((a & b) if name == "and" else (a | b))[m]).all()
    assert_same(oracle_run("eval", cols, LOGIC[name]), want, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LOGIC))
def test_device_truth_tables(ctx, monkeypatch, name):
    base = truth_table_columns()
    idx = np.arange(SITES["k_eval"].n) % len(base[0][0])
    cols = [(v[idx], m[idx]) for v, m in base]
    assert_same(device_run(ctx, monkeypatch, "eval", cols, LOGIC[name]), model_run("eval", cols, LOGIC[name]), name)


# ---- random trees ------------------------------------------------------------------------------------
# columns: 0 Int64, 1 Int32, 2 Float64, 3 Float32, 4 Boolean, 5 Int64
TREE_ROWS, N_TREES, TREE_SEED = 67, 300, 0xE06E
COLUMNS_OF = {em.INT64: [0, 5], em.INT32: [1], em.FLOAT64: [2], em.FLOAT32: [3], em.BOOL: [4]}
TREE_TYPES = [em.INT64, em.INT32, em.FLOAT64, em.FLOAT32, em.BOOL]
FLOAT_EDGES = {
    em.FLOAT64: [0.0, -0.0, 1.5, -1.5, 2.0 ** 53, 2.0 ** 53 + 2, 2.0 ** 63, -2.0 ** 63, 0.1, 1e300, -7.25, 2147483647.5],
    em.FLOAT32: [0.0, -0.0, 1.5, -1.5, 16777216.0, 16777218.0, float(np.float32(0.1)), 3.0e38, -7.25, 2.0 ** 31],
}


def random_literal(r, t):
    if t == em.BOOL:
        return typed_lit(t, bool(r.integers(2)))
    if t in em.INTS:
        e = edge_values(t)
        return typed_lit(t, int(e[r.integers(len(e))]) if r.random() < 0.3 else int(r.integers(-9, 10)))
    e = FLOAT_EDGES[t]
    return typed_lit(t, float(e[r.integers(len(e))]) if r.random() < 0.3 else float(r.integers(-16, 17)) / 4)


def random_tree(r, t, depth, root=False):
    if not root and (depth == 0 or r.random() < 0.25):
        if r.random() < 0.75:
            c = COLUMNS_OF[t]
            return col(c[r.integers(len(c))])
        return random_literal(r, t)
    sub = lambda u: random_tree(r, u, depth - 1)  # noqa: E731
    if t == em.BOOL:
        k = r.random()
        if k < 0.55:
            lt = TREE_TYPES[r.integers(5)]
            rt = em.BOOL if lt == em.BOOL else em.NUMERIC[r.integers(4)]  # every numeric pair coerces
            return binop(sub(lt), list(CMPS.values())[r.integers(6)], sub(rt))
        if k < 0.85:
            return binop(sub(t), BinaryOp.And if r.random() < 0.5 else BinaryOp.Or, sub(t))
        return UnaryExpr(UnaryOp.Not, sub(t))
    if r.random() < 0.12:
        return UnaryExpr(UnaryOp.Minus, sub(t))
    ops = [BinaryOp.Add, BinaryOp.Subtract, BinaryOp.Multiply, BinaryOp.Divide]
    if t in em.INTS:
        ops.append(BinaryOp.Modulo)
    return binop(sub(t), ops[r.integers(len(ops))], sub(t))


def random_table(r, n=TREE_ROWS):
    """half of each column from the type's edge set, half from a small range; about 80 % valid"""
    cols = []
    for t in (em.INT64, em.INT32, em.FLOAT64, em.FLOAT32, em.BOOL, em.INT64):
        edge = r.random(n) < 0.5
        if t in em.INTS:
            e = np.array(edge_values(t), NP_T[t])
            v = np.where(edge, e[r.integers(0, len(e), n)], r.integers(-20, 21, n).astype(NP_T[t]))
        elif t in em.FLOATS:
            e = np.array(FLOAT_EDGES[t], NP_T[t])
            v = np.where(edge, e[r.integers(0, len(e), n)], (r.integers(-64, 65, n) / 8).astype(NP_T[t]))
        else:
            v = r.random(n) < 0.5
        cols.append((v.astype(NP_T[t]), r.random(n) < 0.8))
    return cols


TABLE_TYPES = [em.INT64, em.INT32, em.FLOAT64, em.FLOAT32, em.BOOL, em.INT64]


def device_shape(nodes, column_types=TABLE_TYPES):
    """(instructions, value slots) of the device program for a well-typed postfix: one instruction per
    node plus a conversion for every integer side of a compare that is carried out in Float64."""
    ty, n_ins, depth = [], 0, 0
    for nd in nodes:
        n_ins += 1
        if nd.kind == abi.EX_COLUMN:
            ty.append(column_types[nd.index])
        elif nd.kind == abi.EX_LITERAL:
            ty.append(nd.lit_dtype)
        elif nd.kind == abi.EX_BINARY:
            rt, lt = ty.pop(), ty.pop()
            if nd.op in CMPS.values():
                if lt != rt and (em.FLOAT64 in (lt, rt) or em.FLOAT32 in (lt, rt)):
                    n_ins += (lt in em.INTS) + (rt in em.INTS)
                ty.append(em.BOOL)
            else:
                ty.append(lt)
        depth = max(depth, len(ty))
    return n_ins, depth


@functools.lru_cache(maxsize=None)
def trees():
    """[(expression, columns, the model's outcome)]: seeded; a candidate is left out when its device
    program would pass the limits (those have tests of their own) or when a float operator makes a NaN
    on a valid row (its sign and payload are the hardware's: x86 and gfx950 need not agree)."""
    out, i = [], 0
    while len(out) < N_TREES:
        r = np.random.default_rng([TREE_SEED, i])
        i += 1
        t = TREE_TYPES[r.integers(5)]
        expr = random_tree(r, t, int(r.integers(1, 6)), root=True)
        cols = random_table(r)
        n_ins, depth = device_shape(expr.postfix())
        if n_ins > K_MAX_INSTR or depth > K_NS:
            continue
        try:
            res = em.evaluate_expr(expr, cols)
            if res.saw_nan:
                continue
            assert res.dtype == t
            v, m = res.to_numpy()
            out.append((expr, cols, ("ok", canon(v, m)), t))
        except em.ModelError as e:
            assert e.row >= 0, "the generator makes well-typed trees only: %s" % e
            out.append((expr, cols, ("error", e.status, e.message), t))
    assert i < 3 * N_TREES, "the generator throws too many candidates away (%d for %d)" % (i, N_TREES)
    return out


def test_tree_mix():
    ts = trees()
    raising = sum(w[0] == "error" for _, _, w, _ in ts)
    assert len(ts) >= 300 and raising >= len(ts) // 4 and len(ts) - raising >= len(ts) // 4, (len(ts), raising)
    assert {t for _, _, _, t in ts} == set(TREE_TYPES)
    assert {w[1] for _, _, w, _ in ts if w[0] == "error"} == {abi.QEH_E_OVERFLOW, abi.QEH_E_DIV0}


def test_oracle_random_trees():
    for i, (expr, cols, want, _) in enumerate(trees()):
        assert_same(oracle_run("eval", cols, expr), want, "tree %d: %s" % (i, expr))


@pytest.mark.gpu
def test_device_random_trees_eval(ctx, monkeypatch):
    for i, (expr, cols, want, _) in enumerate(trees()):
        assert_same(device_run(ctx, monkeypatch, "eval", cols, expr), want, "tree %d: %s" % (i, expr))


@pytest.mark.gpu
def test_device_random_trees_filter(ctx):
    """The Boolean trees as predicates: the same error, or the same rows in the same order with every
    column gathered."""
    n_bool = 0
    for i, (expr, cols, want, t) in enumerate(trees()):
        if t != em.BOOL:
            continue
        n_bool += 1
        if want[0] == "ok":
            sel = np.array(want[1][2], bool) & np.array(want[1][1])
            want = ("ok", selection_payload("filter", cols, sel))

        def run():
            out, rows = ctx.filter(upload(ctx, cols), expr)
            return (rows, [canon(*c.to_numpy()) for c in out])
        assert_same(outcome(run), want, "tree %d: %s" % (i, expr))
    assert n_bool >= 30


# ---- first error wins --------------------------------------------------------------------------------
I64_MIN, I64_MAX = em.RANGE[em.INT64]
A, B, C, D = range(4)


def layouts(site):
    """name -> (p, q), p < q: where the two errors of a case sit in the kernel's row layout."""
    s = SITES[site]
    return {
        "same_lane": (5, 5 + s.stride),               # one lane holds both in its `rows` rows
        "same_wave": (3, 10),                          # two lanes of one wave
        "different_blocks": (100, 2 * s.tile + 5),     # tile 0 and the ragged last tile
        "first_and_last_row": (0, s.n - 1),
    }


def benign(n):
    """four valid Int64 columns on which none of the expressions below raises"""
    i = np.arange(n, dtype=np.int64)
    return [i % 7 + 10, np.full(n, 3, np.int64), i % 3 + 2, np.full(n, 5, np.int64)]


def plant(kind, v, row):
    """make a / b raise `kind` at `row`"""
    if kind == "div0":
        v[B][row] = 0
    else:
        v[A][row], v[B][row] = I64_MIN, -1


DIV = binop(col(A), BinaryOp.Divide, col(B))
MOD = binop(col(A), BinaryOp.Modulo, col(B))


@functools.lru_cache(maxsize=None)
def first_error_cases(site):
    """name -> (columns, expression, slice poison or None, the error that wins or None)."""
    s = SITES[site]
    n = s.n
    out = {}

    def add(name, v, expr, wins, valid=None, poison=None):
        valid = valid or {}
        out[name] = ([(x, valid.get(j)) for j, x in enumerate(v)], expr, poison, wins)

    for lname, (p, q) in layouts(site).items():
        for first, second in (("div0", "overflow"), ("overflow", "div0")):
            v = benign(n)
            plant(first, v, p)
            plant(second, v, q)
            add("%s-%s_then_%s" % (lname, first, second), v, DIV, first)
    for sliced_too in (False, True):
        for first, second in (("div0", "overflow"), ("overflow", "div0")):
            v = benign(n)
            plant(first, v, 10)
            plant(second, v, 20)
            va, vb = np.ones(n, bool), np.ones(n, bool)
            v[A][2], v[B][2], va[2] = 1, 0, False           # 1 / 0 under a NULL dividend
            v[A][4], v[B][4], vb[4] = I64_MIN, -1, False    # MIN / -1 under a NULL divisor
            add("%s-%s_then_%s" % ("sliced" if sliced_too else "shielded", first, second), v, DIV, first,
                valid={A: va, B: vb}, poison={B: [0]} if sliced_too else None)  # the parent's other rows: x / 0
    # operator order: the multiplication is the earlier node, so its overflow wins wherever it sits
    mul_div = binop(binop(col(A), BinaryOp.Multiply, col(C)), BinaryOp.Divide, col(B))
    for lname in ("same_lane", "different_blocks"):
        p, q = layouts(site)[lname]
        for mul_row, div_row in ((q, p), (p, q)):
            v = benign(n)
            v[A][mul_row], v[C][mul_row] = 2 ** 62, 4
            v[B][div_row] = 0
            add("operator_order-%s-mul_at_%s" % (lname, "q" if mul_row == q else "p"), v, mul_div, "overflow")
    # remainder: MIN % -1 against a zero divisor and against an overflow, either node first, either row first
    p, q = layouts(site)["different_blocks"]
    div_cd = binop(col(C), BinaryOp.Divide, col(D))
    add_cd = binop(col(C), BinaryOp.Add, col(D))
    for other, oname in ((div_cd, "div0"), (add_cd, "overflow")):
        for mod_first in (True, False):
            for mod_row, other_row in ((p, q), (q, p)):
                v = benign(n)
                v[A][mod_row], v[B][mod_row] = I64_MIN, -1
                if oname == "div0":
                    v[D][other_row] = 0
                else:
                    v[C][other_row], v[D][other_row] = I64_MAX, 1
                expr = binop(MOD, BinaryOp.Add, other) if mod_first else binop(other, BinaryOp.Add, MOD)
                add("remainder-%s_node_%s-mod_row_%s" % (oname, "second" if mod_first else "first",
                                                         "p" if mod_row == p else "q"),
                    v, expr, "remainder" if mod_first else oname)
    # a zero divisor makes a % b NULL, and the NULL feeds on: no error where a + MAX would overflow
    v = benign(n)
    v[A] = -(np.arange(n, dtype=np.int64) % 5)
    v[B][:] = 7
    for row in (0, 5, 5 + s.stride, 100, 2 * s.tile + 5, n - 1):
        v[A][row], v[B][row] = 5, 0
    add("mod_by_zero_feeds_on", v, binop(MOD, BinaryOp.Add, lit(I64_MAX)), None)
    return out


WINS = {"div0": (abi.QEH_E_DIV0, em.MSG_DIV0), "overflow": (abi.QEH_E_OVERFLOW, em.MSG_OVERFLOW),
        "remainder": (abi.QEH_E_OVERFLOW, em.MSG_REMAINDER)}
CASE_NAMES = sorted(first_error_cases("k_eval"))


def expected_first_error(site, form, name):
    cols, expr, poison, wins = first_error_cases(site)[name]
    want = model_run(form, cols, expr)
    if wins is None:
        assert want[0] == "ok"
    else:
        assert want == ("error",) + WINS[wins], (name, want)
    return cols, expr, poison, want


@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("site,form", SITE_FORMS)
def test_oracle_first_error_wins(site, form, name):
    cols, expr, _, want = expected_first_error(site, form, name)
    assert_same(oracle_run(form, cols, expr), want, name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASE_NAMES)
@pytest.mark.parametrize("site,form", SITE_FORMS)
def test_device_first_error_wins(ctx, monkeypatch, site, form, name):
    cols, expr, poison, want = expected_first_error(site, form, name)
    assert_same(device_run(ctx, monkeypatch, form, cols, expr, slice_poison=poison), want, name)


# ---- program limits ----------------------------------------------------------------------------------

def right_nested_sum(k):
    e = col(k - 1)
    for j in range(k - 2, -1, -1):
        e = binop(col(j), BinaryOp.Add, e)
    return e


def left_chain(k):
    """-c0 + 1 + 1 ...: 2 + 2k instructions"""
    e = UnaryExpr(UnaryOp.Minus, col(0))
    for _ in range(k):
        e = binop(e, BinaryOp.Add, lit(1))
    return e


def limit_columns(k, n):
    r = np.random.default_rng(k)
    return [(r.integers(-1000, 1000, n).astype(np.int64), r.random(n) < 0.9) for _ in range(k)]


TOO_DEEP = (abi.QEH_E_UNSUPPORTED, "expression too deep")
TOO_LARGE = (abi.QEH_E_UNSUPPORTED, "expression too large for the device program (max %d instructions)" % K_MAX_INSTR)


def test_limit_expressions_sit_at_the_limits():
    shape = lambda e: device_shape(e.postfix(), [em.INT64] * (K_NS + 1))  # noqa: E731
    assert shape(right_nested_sum(K_NS)) == (2 * K_NS - 1, K_NS)
    assert shape(right_nested_sum(K_NS + 1))[1] == K_NS + 1
    assert shape(left_chain(19)) == (K_MAX_INSTR, 2)
    assert shape(forty_one_instructions()) == (K_MAX_INSTR + 1, 2)
    conj = ten_term_conjunction()
    assert len(conj.postfix()) == 39 and shape(conj)[0] == 49


def forty_one_instructions():
    """-(-c0 + 1 ... + 1) with 19 additions: the chain of exactly 40 instructions and one more"""
    return UnaryExpr(UnaryOp.Minus, left_chain(19))


def ten_term_conjunction():
    e = binop(col(0), BinaryOp.Less, lit(1.5))
    for _ in range(9):
        e = e & binop(col(0), BinaryOp.Less, lit(1.5))
    return e


@pytest.mark.gpu
def test_device_program_at_the_limits(ctx, monkeypatch):
    """Stack depth 8 (the slot accessors' default arm) and exactly 40 instructions: the model's result."""
    n = SITES["k_eval"].n
    cols = limit_columns(K_NS, n)
    for expr in (right_nested_sum(K_NS), left_chain(19)):
        want = model_run("eval", cols, expr)
        assert want[0] == "ok"
        assert_same(device_run(ctx, monkeypatch, "eval", cols, expr), want, str(expr))
    for form in ("filter", "agg_no_key", "agg_key_lds", "agg_key_table"):
        expr = right_nested_sum(K_NS)
        assert_same(device_run(ctx, monkeypatch, form, cols, expr), model_run(form, cols, expr), form)


@pytest.mark.gpu
def test_device_program_past_the_limits_is_refused(ctx, monkeypatch):
    """Depth 9, 41 instructions, and ten `int_col < 1.5` terms (39 nodes, 49 instructions with the
    hidden conversions): refused by name in every form, never a wrong result."""
    n = 100
    cols = limit_columns(K_NS + 1, n)
    for form in ("eval", "filter", "agg_no_key", "agg_key_lds"):
        got = device_run(ctx, monkeypatch, form, cols, right_nested_sum(K_NS + 1))
        assert got == ("error",) + TOO_DEEP, (form, got)
        got = device_run(ctx, monkeypatch, form, cols, forty_one_instructions())
        assert got == ("error",) + TOO_LARGE, (form, got)

    def conj(run):
        return outcome(lambda: run(upload(ctx, cols), ten_term_conjunction()))
    assert conj(ctx.eval) == ("error",) + TOO_LARGE
    assert conj(ctx.filter) == ("error",) + TOO_LARGE
    assert conj(lambda dev, e: ctx.filter_aggregate(dev, e, [], [(AF.Count, 0)])) == ("error",) + TOO_LARGE
