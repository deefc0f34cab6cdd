"""An exact model of the reference's expression semantics, written from the reference's source
(crates/query-executor/src/operators.rs; the line numbers below are that file's) and from nothing
else of this project: it shares only the postfix node encoding (`PhysicalExpr.postfix()` ->
`abi.QehExprNode`) and the enum values of include/qeh.h with the code under test.  Pure Python: the
integers are Python's big ints checked against the type's range, Float64 values are numpy float64
scalars, Float32 values are rounded through numpy.float32 after every operation.

`evaluate` walks the postfix nodes as `evaluate_expr` (:13-62) recurses: operands first, left before
right, and every operator finishes its whole array -- rows in order, NULL rows skipped -- before the
next one starts.  The first error it meets is therefore the one with the least (post-order node index,
row) among the valid rows that raise, and that is the error it raises (`ModelError`).  A type error
belongs to its node as a whole (row -1): it is met when that node is evaluated, after every error of
the nodes before it.

Texts: arrow's errors are prefixed "Arrow error: " by the reference's error type; this project fixed
the texts of the three value errors (include/qeh.h), and the model states those."""
import numpy as np

from qe_hip import abi

NULL, BOOL, INT32, INT64, FLOAT32, FLOAT64 = (abi.DT_NULL, abi.DT_BOOL, abi.DT_INT32, abi.DT_INT64,
                                              abi.DT_FLOAT32, abi.DT_FLOAT64)
INTS, FLOATS = (INT32, INT64), (FLOAT32, FLOAT64)
NUMERIC = INTS + FLOATS
RANGE = {INT32: (-2 ** 31, 2 ** 31 - 1), INT64: (-2 ** 63, 2 ** 63 - 1)}
BITS = {INT32: 32, INT64: 64}
NAME = {NULL: "Null", BOOL: "Boolean", INT32: "Int32", INT64: "Int64", FLOAT32: "Float32", FLOAT64: "Float64"}
NP_OF = {BOOL: np.bool_, INT32: np.int32, INT64: np.int64, FLOAT32: np.float32, FLOAT64: np.float64, NULL: np.int64}

MSG_DIV0 = "Arrow error: Divide by zero error"
MSG_OVERFLOW = "Arrow error: Arithmetic overflow"
MSG_REMAINDER = "attempt to calculate the remainder with overflow (the reference aborts here, operators.rs:720)"
ARITH_NAME = {abi.OP_ADD: "addition", abi.OP_SUB: "subtraction", abi.OP_MUL: "multiplication", abi.OP_DIV: "division"}
CMP_SYM = {abi.OP_EQ: "==", abi.OP_NEQ: "!=", abi.OP_LT: "<", abi.OP_LTE: "<=", abi.OP_GT: ">", abi.OP_GTE: ">="}


class ModelError(Exception):
    def __init__(self, status, message, node_index, row):
        super().__init__("[%s] %s (node %d, row %d)" % (abi.STATUS_NAMES.get(status, status), message, node_index, row))
        self.status, self.message, self.node_index, self.row = status, message, node_index, row


class Array:
    """One evaluated node: `dtype`, a Python list of values (ints, 0/1 for Boolean, numpy.float64 for
    both float types) and a list of validity flags.  The value of a NULL row is not part of the result."""

    def __init__(self, dtype, values, valid):
        self.dtype, self.values, self.valid = dtype, values, valid

    def to_numpy(self):
        """(values in the type's numpy dtype, bool validity); a NullArray reads as all-NULL Int64."""
        vals = [v if ok else 0 for v, ok in zip(self.values, self.valid)]
        with np.errstate(all="ignore"):
            out = np.array(vals, np.float64 if self.dtype in FLOATS else np.int64).astype(NP_OF[self.dtype])
        return out, np.array(self.valid, bool)


class Result(Array):
    """The root's array; `saw_nan`: some float operator produced a NaN on a valid row (the sign and
    payload of such a NaN are the hardware's choice, so a test may want to leave that tree out)."""
    saw_nan = False


def _column(values, valid):
    values = np.asarray(values)
    n = len(values)
    ok = [True] * n if valid is None else [bool(v) for v in valid]
    kind = values.dtype.kind
    if kind == "b":
        return Array(BOOL, [int(v) for v in values], ok)
    if kind == "i":
        return Array({4: INT32, 8: INT64}[values.dtype.itemsize], [int(v) for v in values], ok)
    if kind == "f":
        return Array({4: FLOAT32, 8: FLOAT64}[values.dtype.itemsize], [np.float64(v) for v in values], ok)
    raise TypeError(values.dtype)


def _literal(nd, n):
    # create_literal_array (:322-347): the value n times; ScalarValue::Null and typed None -> NullArray
    t = NULL if nd.lit_is_null else nd.lit_dtype
    if t == NULL:
        return Array(NULL, [0] * n, [False] * n)
    if t == FLOAT64:
        v = np.float64(nd.lit_f64)
    elif t == FLOAT32:
        with np.errstate(all="ignore"):
            v = np.float64(np.float32(nd.lit_f64))
    elif t == BOOL:
        v = int(nd.lit_i64 != 0)
    elif t == INT32:
        v = (int(nd.lit_i64) + 2 ** 31) % 2 ** 32 - 2 ** 31
    elif t == INT64:
        v = int(nd.lit_i64)
    else:
        raise TypeError("literal dtype %d" % t)
    return Array(t, [v] * n, [True] * n)


def _wrap(x, t):
    half = 2 ** (BITS[t] - 1)
    return (x + half) % (2 * half) - half


def _trunc_div(a, b):
    q = abs(a) // abs(b)
    return -q if (a < 0) != (b < 0) else q


def total_order_key(x):
    """IEEE 754 totalOrder as a signed integer (arrow's float comparisons, kernels::cmp)."""
    b = int(np.float64(x).view(np.int64))
    return b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFF)


def _to_f64(a):
    # `x as f64` (:630-646, cast_to_float64 :678-709): Float32 widens exactly, integers round to nearest even
    if a.dtype in INTS:
        return Array(FLOAT64, [np.float64(float(v)) for v in a.values], a.valid)
    if a.dtype == FLOAT32:
        return Array(FLOAT64, a.values, a.valid)
    return a


def _coerce(l, r):
    # coerce_numeric_types (:616-675), in its order
    if l.dtype == r.dtype:
        return l, r
    if l.dtype == FLOAT64 and r.dtype in INTS:
        return l, _to_f64(r)
    if r.dtype == FLOAT64 and l.dtype in INTS:
        return _to_f64(l), r
    if FLOAT32 in (l.dtype, r.dtype):
        return _to_f64(l), _to_f64(r)
    if l.dtype == INT64 and r.dtype == INT32:
        return l, Array(INT64, r.values, r.valid)
    if r.dtype == INT64 and l.dtype == INT32:
        return Array(INT64, l.values, l.valid), r
    return l, r  # ":673 let Arrow handle the error"


def _unary(op, a, i):
    if op == abi.UOP_NOT:  # :351-359, compute::not keeps the validity
        if a.dtype != BOOL:
            raise ModelError(abi.QEH_E_TYPE, "NOT operator requires boolean array", i, -1)
        return Array(BOOL, [1 - v for v in a.values], a.valid)
    # :360-378: `-x` per valid row; a release build wraps the integers
    if a.dtype in INTS:
        return Array(a.dtype, [_wrap(-v, a.dtype) for v in a.values], a.valid)
    if a.dtype in FLOATS:
        return Array(a.dtype, [np.negative(v) for v in a.values], a.valid)
    raise ModelError(abi.QEH_E_TYPE, "Unsupported type for negation", i, -1)


def _float_op(op, t, x, y):
    with np.errstate(all="ignore"):
        if t == FLOAT32:
            x, y = np.float32(x), np.float32(y)
        z = x + y if op == abi.OP_ADD else x - y if op == abi.OP_SUB else x * y if op == abi.OP_MUL else x / y
        return np.float64(z)


def _arith(op, l, r, i, res):
    # :384-507: both sides of one numeric type, no coercion; arrow's add / sub / mul / div are the
    # checked kernels (try_binary: valid rows only, in order, the first error returns)
    if l.dtype != r.dtype or l.dtype not in NUMERIC:
        raise ModelError(abi.QEH_E_TYPE, "Unsupported types for " + ARITH_NAME[op], i, -1)
    t, n = l.dtype, len(l.values)
    valid = [a and b for a, b in zip(l.valid, r.valid)]
    out = [0] * n
    if t in FLOATS:
        for k in range(n):
            out[k] = _float_op(op, t, l.values[k], r.values[k])
            if valid[k] and np.isnan(out[k]) and not (np.isnan(l.values[k]) or np.isnan(r.values[k])):
                res.saw_nan = True
        return Array(t, out, valid)
    lo, hi = RANGE[t]
    for k in range(n):
        if not valid[k]:
            continue
        a, b = l.values[k], r.values[k]
        if op == abi.OP_DIV:
            if b == 0:  # div_checked: the zero divisor is looked at first
                raise ModelError(abi.QEH_E_DIV0, MSG_DIV0, i, k)
            if a == lo and b == -1:
                raise ModelError(abi.QEH_E_OVERFLOW, MSG_OVERFLOW, i, k)
            z = _trunc_div(a, b)
        else:
            z = a + b if op == abi.OP_ADD else a - b if op == abi.OP_SUB else a * b
            if z < lo or z > hi:
                raise ModelError(abi.QEH_E_OVERFLOW, MSG_OVERFLOW, i, k)
        out[k] = z
    return Array(t, out, valid)


def _modulo(l, r, i):
    # modulo_op (:711-743): (Some(l), Some(r)) if r != 0 => Some(l % r), else None; `%` truncates,
    # and MIN % -1 is Rust's "attempt to calculate the remainder with overflow"
    if l.dtype != r.dtype or l.dtype not in INTS:
        raise ModelError(abi.QEH_E_TYPE, "Modulo operation requires integer arrays", i, -1)
    t, n = l.dtype, len(l.values)
    out, valid = [0] * n, [False] * n
    for k in range(n):
        a, b = l.values[k], r.values[k]
        if not (l.valid[k] and r.valid[k]) or b == 0:
            continue
        if a == RANGE[t][0] and b == -1:
            raise ModelError(abi.QEH_E_OVERFLOW, MSG_REMAINDER, i, k)
        out[k], valid[k] = a - b * _trunc_div(a, b), True
    return Array(t, out, valid)


def _compare(op, l, r, i):
    # :509-538: coerce, then arrow's eq / neq / lt / lt_eq / gt / gt_eq (floats by totalOrder)
    l, r = _coerce(l, r)
    if l.dtype != r.dtype or l.dtype == NULL:
        raise ModelError(abi.QEH_E_TYPE, "Invalid argument error: Invalid comparison operation: %s %s %s"
                         % (NAME[l.dtype], CMP_SYM[op], NAME[r.dtype]), i, -1)
    key = total_order_key if l.dtype in FLOATS else int
    out = []
    for a, b in zip(l.values, r.values):
        a, b = key(a), key(b)
        out.append(int({abi.OP_EQ: a == b, abi.OP_NEQ: a != b, abi.OP_LT: a < b, abi.OP_LTE: a <= b,
                        abi.OP_GT: a > b, abi.OP_GTE: a >= b}[op]))
    return Array(BOOL, out, [x and y for x, y in zip(l.valid, r.valid)])


def _logical(op, l, r, i):
    # :539-570: arrow's non-Kleene compute::and / or -- NULL if either side is NULL
    if l.dtype != BOOL or r.dtype != BOOL:
        raise ModelError(abi.QEH_E_TYPE, "AND requires boolean arrays" if op == abi.OP_AND else "OR requires boolean arrays", i, -1)
    f = (lambda a, b: a & b) if op == abi.OP_AND else (lambda a, b: a | b)
    return Array(BOOL, [f(a, b) for a, b in zip(l.values, r.values)], [x and y for x, y in zip(l.valid, r.valid)])


def evaluate(nodes, cols, n_rows):
    """`nodes`: abi.QehExprNode sequence in postfix order.  `cols`: (numpy values, validity-or-None)
    pairs.  Returns a Result or raises ModelError for the reference's first error."""
    res = Result(NULL, [], [])
    stack = []
    for i, nd in enumerate(nodes):
        if nd.kind == abi.EX_COLUMN:
            if nd.index < 0 or nd.index >= len(cols):  # :16-21
                raise ModelError(abi.QEH_E_INVALID, "Column index %d out of bounds" % nd.index, i, -1)
            stack.append(_column(*cols[nd.index]))
        elif nd.kind == abi.EX_LITERAL:
            stack.append(_literal(nd, n_rows))
        elif nd.kind == abi.EX_UNARY:
            stack.append(_unary(nd.op, stack.pop(), i))
        elif nd.kind == abi.EX_BINARY:
            r, l = stack.pop(), stack.pop()
            if nd.op in ARITH_NAME:
                stack.append(_arith(nd.op, l, r, i, res))
            elif nd.op == abi.OP_MOD:
                stack.append(_modulo(l, r, i))
            elif nd.op in CMP_SYM:
                stack.append(_compare(nd.op, l, r, i))
            elif nd.op in (abi.OP_AND, abi.OP_OR):
                stack.append(_logical(nd.op, l, r, i))
            else:
                raise NotImplementedError("binary operator %d" % nd.op)
        else:
            raise NotImplementedError("node kind %d" % nd.kind)
    (root,) = stack
    res.dtype, res.values, res.valid = root.dtype, root.values, root.valid
    return res


def evaluate_expr(expr, cols, n_rows=None):
    return evaluate(expr.postfix(), cols, len(cols[0][0]) if n_rows is None else n_rows)
