"""CSV scan on the device (qeh_scan_csv, qeh_source_cache_load_csv; DESIGN.md §4 "CSV scan").

CPU half: the cell parsers of csrc/parse_float.h built for the host (tests/parse_host.cpp) against
Python's float() / int() / datetime.date; the plain-Python model of the dialect (tests/csv_model.py)
against hand-written answers and against pyarrow.csv on inputs both read alike; the ABI declaration.
GPU half: the device reader must equal the model exactly -- values, validity, offsets, null_count --
or refuse at the model's (row, column); the employees / departments plan over preloaded CSV sources."""
import ctypes as C
import datetime
import io
import os
import random
import re
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pyarrow as pa
import pyarrow.csv as pacsv
import pytest

import csv_model as M
import qe_hip
from qe_hip import (AggregateExpr, AggregateFunction as AF, BinaryOp, CsvDataSource, Filter, HashAggregate, HashJoin,
                    JoinType, MemoryDataSource, Projection, QueryExecutor, Scan, abi, binop, lit)
from qe_hip.expr import Column

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")

ARROW_OF = {M.INT32: pa.int32(), M.INT64: pa.int64(), M.FLOAT64: pa.float64(), M.BOOL: pa.bool_(), M.DATE32: pa.date32(),
            M.UTF8: pa.string()}
ALL_SIX = [M.INT32, M.INT64, M.FLOAT64, M.BOOL, M.DATE32, M.UTF8]


def schema_of(dtypes):
    return pa.schema([pa.field(f"c{i}", ARROW_OF[d]) for i, d in enumerate(dtypes)])


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def f64_of_bits(u):
    return struct.unpack("<d", struct.pack("<Q", u))[0]


# ---- float cells: the list both halves use ---------------------------------------------------------

def halfway_cells(rng, count):
    """Exact midpoints of adjacent doubles, written out in full (positional and with an exponent)."""
    out = []
    for _ in range(count):
        e = rng.choice([0, 1, 2, 10, 900, 1000, 1022, 1023, 1024, 1030, 1075, 1100, 1200, 2000])
        u = (e << 52) | rng.getrandbits(52)
        mid = (Fraction(f64_of_bits(u)) + Fraction(f64_of_bits(u + 1))) / 2
        num, den, k = mid.numerator, mid.denominator, 0
        while den % 2 == 0:
            den //= 2
            k += 1
        assert den == 1
        digits = str(num * 5 ** k)
        out.append(f"{digits}e-{k}" if k else digits)
        if len(digits) > k > 0:
            out.append(digits[:-k] + "." + digits[-k:])
    return out


def edge_float_cells():
    rng = random.Random(7)
    cells = ["9007199254740993", "1.7976931348623158e308", "1.7976931348623159e308", "8.5e-324", "4.9e-324",
             "2.4703282292062327e-324", "2.4703282292062328e-324", "2.2250738585072011e-308", "2.2250738585072014e-308",
             "0.500000000000000166533453693773481063544750213623046875", "9007199254740992.5", "9007199254740993.5",
             "9007199254740992.50000000000000000000001", "0", "-0", "-0.0", "0e999", "1e-400", "1e400", "-1e400", "1.", ".5",
             "1.e5", "007.50", "nan", "NaN", "-nan", "inf", "-Inf", "INFINITY", "-infinity",
             "12345678901234567", "1234567890123456789", "12345678901234567890",  # 17, 19, 20 digits
             "1234567890123456789012345678901234567890", "0.1234567890123456789012345678901234567890",
             "1" + "0" * 30, "0." + "0" * 30 + "1", "123456789012345678901234567890e-50"]
    for e in (22, 23, 308):
        cells += [f"1e{e}", f"1e-{e}", f"9007199254740991e{e}", f"9007199254740991e-{e}", f"1.5E+{e}"]
    cells += ["1e-324", "3e-324", "5e-324"]
    for k in range(-1074, 1024):  # every power of two and its neighbours
        base = f64_bits(2.0 ** k)
        for d in (-1, 0, 1):
            if 0 < base + d < 0x7FF0000000000000:
                cells.append(repr(f64_of_bits(base + d)))
    for u in range(1, 1 << 14, 5):  # subnormals below 2^-1060
        cells.append(repr(f64_of_bits(u)))
    return cells + halfway_cells(rng, 150)


def random_reprs(count, seed=1):
    rng = random.Random(seed)
    out = []
    while len(out) < count:
        x = f64_of_bits(rng.getrandbits(64))
        if x == x and abs(x) != float("inf"):
            out.append(repr(x))
    return out


# ---- CPU: the cell parsers ------------------------------------------------------------------------

@pytest.fixture(scope="module")
def parsers(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("parse") / "parse_host.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "parse_host.cpp"),
                           "-I", os.path.join(ROOT, "query-engine_amd", "csrc"), "-o", so])
    lib = C.CDLL(so)
    lib.parse_f64_c.argtypes = [C.c_char_p, C.c_longlong, C.POINTER(C.c_ulonglong)]
    lib.parse_int_c.argtypes = [C.c_char_p, C.c_longlong, C.c_ulonglong, C.POINTER(C.c_longlong)]
    lib.parse_date32_c.argtypes = [C.c_char_p, C.c_longlong, C.POINTER(C.c_int)]
    return lib


def host_f64(lib, s):
    b = C.c_ulonglong()
    r = lib.parse_f64_c(s.encode(), len(s), C.byref(b))
    return r, b.value


def test_float_parser_on_shortest_reprs(parsers):
    """Every shortest repr is either Python's double bit for bit or "cannot decide", and at most
    1 % are the latter (observed: none of 150 000)."""
    cells = random_reprs(150_000)
    undecided = 0
    for s in cells:
        r, b = host_f64(parsers, s)
        if r == 1:
            undecided += 1
        else:
            assert r == 0 and b == f64_bits(float(s)), (s, r, hex(b))
    print(f"undecided share among {len(cells)} shortest reprs: {undecided / len(cells):.6f}")
    assert undecided <= len(cells) // 100


def test_float_parser_on_edges(parsers):
    decided = 0
    for s in edge_float_cells():
        r, b = host_f64(parsers, s)
        assert r in (0, 1), s
        if r == 0:
            decided += 1
            assert b == f64_bits(float(s)), (s, hex(b), hex(f64_bits(float(s))))
    assert decided > 6000  # "cannot decide" is for the long halfway cases, not a way out
    assert host_f64(parsers, "9007199254740993") == (0, f64_bits(9007199254740992.0))
    assert host_f64(parsers, "1.7976931348623159e308") == (0, 0x7FF0000000000000)
    assert host_f64(parsers, "8.5e-324") == (0, 2)
    assert host_f64(parsers, "-nan") == (0, 0xFFF8000000000000)
    assert host_f64(parsers, "-0") == (0, 1 << 63)


def test_float_grammar(parsers):
    for s in ["", "-", "+5", " 5", "5 ", "1e", "1e+", "e5", ".", "1..2", "1_0", "0x10", "infinit", "nan(1)", "--1", "1e5.0"]:
        assert host_f64(parsers, s)[0] == 2, s
        if s:  # (an empty cell never reaches the grammar: it is NULL)
            with pytest.raises(M._Broken):
                M.cell_value(M.FLOAT64, s.encode())


def test_int_and_date_parsers(parsers):
    v = C.c_longlong()
    for s, mx, want in [("0", 2**63 - 1, 0), ("-0", 2**63 - 1, 0), ("007", 2**31 - 1, 7), ("9223372036854775807", 2**63 - 1, 2**63 - 1),
                        ("-9223372036854775808", 2**63 - 1, -2**63), ("9223372036854775808", 2**63 - 1, None),
                        ("-9223372036854775809", 2**63 - 1, None), ("2147483647", 2**31 - 1, 2**31 - 1),
                        ("2147483648", 2**31 - 1, None), ("-2147483648", 2**31 - 1, -2**31), ("-2147483649", 2**31 - 1, None),
                        ("+5", 2**63 - 1, None), ("1.5", 2**63 - 1, None), ("", 2**63 - 1, None), ("-", 2**63 - 1, None),
                        ("0" * 40 + "12", 2**31 - 1, 12), ("99999999999999999999999", 2**63 - 1, None)]:
        r = parsers.parse_int_c(s.encode(), len(s), mx, C.byref(v))
        assert (r, v.value if r == 0 else None) == ((0, want) if want is not None else (2, None)), s
    d = C.c_int()
    rng = random.Random(3)
    days = [-719162, 2932896, 0, -1, 59, 60, 11016, 11017] + [rng.randrange(-719162, 2932897) for _ in range(5000)]
    for n in days:
        s = (datetime.date(1970, 1, 1) + datetime.timedelta(days=n)).isoformat()
        assert parsers.parse_date32_c(s.encode(), len(s), C.byref(d)) == 0 and d.value == n, s
    for s in ["2023-02-30", "2023-2-3", "0000-01-01", "2023-13-01", "2023-00-10", "2023-01-00", "1900-02-29", "2023/01/01",
              "2023-01-011", "20230101  "]:
        assert parsers.parse_date32_c(s.encode(), len(s), C.byref(d)) == 2, s
    s = "2000-02-29"
    assert parsers.parse_date32_c(s.encode(), len(s), C.byref(d)) == 0 and d.value == 11016


def test_prototype_is_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "qeh.h")).read()
    assert "#define QEH_ABI_VERSION 1" in src  # additive change
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"^\s*int\s+qeh_scan_csv\s*\(([^)]*)\)\s*;", code, flags=re.M)
    assert m, "qeh_scan_csv is not declared in include/qeh.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["qeh_ctx *ctx", "const uint8_t *bytes", "int64_t size", "int bytes_on_device", "int has_header",
                    "const int32_t *dtypes", "int n_cols", "qeh_column *out_cols", "int64_t *out_rows"], args
    plan = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "qeh_plan.h")).read(), flags=re.S)
    assert re.search(r"^\s*int\s+qeh_source_cache_load_csv\s*\(", plan, flags=re.M)
    for name, n_args in (("qeh_scan_csv", 9), ("qeh_source_cache_load_csv", 9)):
        restype, argtypes = abi.SIGNATURES[name]
        assert restype is C.c_int and len(argtypes) == n_args
        assert hasattr(qe_hip.load(), name)
        out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], capture_output=True, text=True).stdout
        assert re.search(rf"\b{name}\b", out)
    assert hasattr(qe_hip.Context, "scan_csv") and hasattr(CsvDataSource, "preload")
    assert qe_hip.load().qeh_abi_version() == 1


# ---- documents -----------------------------------------------------------------------------------

WORDS = ["x", "Alice", "a b", "naïve", "日本語", "😀 smile", "tab\there", "O'Brien", "-", "NULL", "0", "é"]


def cell_text(rng, dtype, null_share):
    """One cell of a column: (text of the content, must-quote)."""
    if rng.random() < null_share:
        return "", False
    if dtype == M.INT32:
        return str(rng.choice([0, -1, 7, 2**31 - 1, -2**31, rng.randrange(-10**6, 10**6)])), False
    if dtype == M.INT64:
        return str(rng.choice([0, 2**63 - 1, -2**63, rng.randrange(-10**15, 10**15)])), False
    if dtype == M.FLOAT64:
        return repr(f64_of_bits(rng.getrandbits(64) % 0x7FF0000000000000)), False
    if dtype == M.BOOL:
        return rng.choice(["true", "false", "True", "False", "TRUE", "FALSE"]), False
    if dtype == M.DATE32:
        return (datetime.date(1970, 1, 1) + datetime.timedelta(days=rng.randrange(-719162, 2932897))).isoformat(), False
    w = rng.choice(WORDS)
    k = rng.random()
    if k < 0.15:
        return w + "," + w, True
    if k < 0.25:
        return w + "\n" + w, True
    if k < 0.32:
        return 'say "' + w + '"', True
    if k < 0.38:
        return "line\r\nbreak", True
    return w, False


def document(rng, dtypes, n_rows, terminators=("\n",), null_share=0.15, quote_share=0.2, header=True, last_terminated=True,
             blank_lines=False):
    lines = []
    if header:
        lines.append(",".join(f"c{i}" for i in range(len(dtypes))))
    for _ in range(n_rows):
        cells = []
        for dt in dtypes:
            text, must = cell_text(rng, dt, null_share)
            if must or rng.random() < quote_share:
                text = '"' + text.replace('"', '""') + '"'
            cells.append(text)
        if len(dtypes) == 1 and cells[0] == "":
            cells[0] = '""'  # an unquoted empty single field would be a record without bytes
        lines.append(",".join(cells))
    out = ""
    for i, ln in enumerate(lines):
        out += ln
        if i + 1 < len(lines) or last_terminated:
            out += rng.choice(terminators)
            if blank_lines and rng.random() < 0.3:
                out += rng.choice(terminators) * rng.randrange(1, 3)
    return out.encode()


def arrow_table(data, dtypes, has_header=True):
    names = [f"c{i}" for i in range(len(dtypes))]
    return pacsv.read_csv(
        io.BytesIO(data), read_options=pacsv.ReadOptions(column_names=names, skip_rows=1 if has_header else 0),
        parse_options=pacsv.ParseOptions(newlines_in_values=True),
        convert_options=pacsv.ConvertOptions(
            column_types={n: ARROW_OF[d] for n, d in zip(names, dtypes)}, null_values=[""], strings_can_be_null=True,
            quoted_strings_can_be_null=True, true_values=["true", "True", "TRUE"], false_values=["false", "False", "FALSE"]))


def assert_model_equals_arrow(model, table, dtypes):
    assert table.num_columns == len(dtypes)
    for (values, valid), dt, col in zip(model, dtypes, table.columns):
        got = col.to_pylist()
        assert len(got) == len(values)
        for v, ok, g in zip(values, valid, got):
            if not ok:
                assert g is None
            elif dt == M.FLOAT64:
                assert g is not None and f64_bits(g) == f64_bits(v), (v, g)
            elif dt == M.DATE32:
                assert g == datetime.date(1970, 1, 1) + datetime.timedelta(days=v)
            elif dt == M.UTF8:
                assert g is not None and g.encode() == v
            else:
                assert g == v


# (name, bytes, dtypes, has_header, the answer by hand or None, compare with pyarrow)
def dialect_documents():
    rng = random.Random(11)
    docs = [
        ("empty input", b"", [M.INT64], True, [([], [])], False),
        ("header only, terminated", b"a,b\n", [M.INT64, M.UTF8], True, [([], []), ([], [])], False),
        ("header only, open", b"a,b", [M.INT64, M.UTF8], True, [([], []), ([], [])], False),
        ("one row", b"a,b\n1,x\n", [M.INT64, M.UTF8], True, [([1], [True]), ([b"x"], [True])], True),
        ("last record open", b"a,b\n1,x\n2,y", [M.INT64, M.UTF8], True, [([1, 2], [True, True]), ([b"x", b"y"], [True, True])],
         True),
        ("no header", b"1,x\n2,y\n", [M.INT64, M.UTF8], False, [([1, 2], [True, True]), ([b"x", b"y"], [True, True])], True),
        ("nulls quoted and not", b'a,b\n,""\n"",\n', [M.INT64, M.UTF8], True, [([0, 0], [False, False]), ([b"", b""], [False, False])],
         True),
        ("cr, crlf and lf", b"a\r1\r\n2\n3\r", [M.INT32], True, [([1, 2, 3], [True] * 3)], True),
        # (pyarrow's skip_rows counts the blank lines in front of the header: not compared)
        ("blank lines", b"\n\na\n\n1\n\r\n\r\n2\n\n", [M.INT32], True, [([1, 2], [True] * 2)], False),
        ("blank lines after the header", b"a\n\n1\n\r\n\r\n2\n\n", [M.INT32], True, [([1, 2], [True] * 2)], True),
        ("quote-only lines", b'a\n""\n1\n""\n', [M.INT32], True, [([0, 1, 0], [False, True, False])], False),
        ("quoted structure", b'a,b\n"x,y","l1\nl2"\n"r\r\nn","say ""hi"""\n""""," "\n', [M.UTF8, M.UTF8], True,
         [([b"x,y", b"r\r\nn", b'"'], [True] * 3), ([b"l1\nl2", b'say "hi"', b" "], [True] * 3)], True),
        ("multi-byte", 'a,b\nnaïve,"日本語"\n"😀",é\n'.encode(), [M.UTF8, M.UTF8], True,
         [(["naïve".encode(), "😀".encode()], [True] * 2), (["日本語".encode(), "é".encode()], [True] * 2)], True),
        ("trailing delimiter is a field", b"a,b\n1,\n", [M.INT64, M.INT64], True, [([1], [True]), ([0], [False])], True),
        ("integers", b"a,b\n-0,007\n-9223372036854775808,2147483647\n9223372036854775807,-2147483648\n", [M.INT64, M.INT32], True,
         [([0, -2**63, 2**63 - 1], [True] * 3), ([7, 2**31 - 1, -2**31], [True] * 3)], True),
        ("booleans", b"a\ntrue\nFALSE\nTrue\n", [M.BOOL], True, [([True, False, True], [True] * 3)], True),
        ("odd-case booleans", b"a\ntRuE\nfalsE\n", [M.BOOL], True, [([True, False], [True] * 2)], False),
        ("dates", b"a\n1970-01-01\n0001-01-01\n9999-12-31\n2000-02-29\n", [M.DATE32], True,
         [([0, -719162, 2932896, 11016], [True] * 4)], True),
        ("floats", b"a\n1.5\n-0\n1e3\n.5\n9007199254740993\n", [M.FLOAT64], True,
         [([1.5, -0.0, 1000.0, 0.5, 9007199254740992.0], [True] * 5)], True),
    ]
    for n in (1, 63, 64, 65, 257):
        docs.append((f"all six, {n} rows", document(rng, ALL_SIX, n), ALL_SIX, True, None, True))
    for dt in ALL_SIX:
        docs.append((f"{dt} alone", document(rng, [dt], 130), [dt], True, None, dt != M.UTF8 and dt != M.BOOL))
        docs.append((f"{dt} all null", document(rng, [dt], 70, null_share=1.0), [dt], True, None, False))
        docs.append((f"{dt} no null", document(rng, [dt, dt], 70, null_share=0.0), [dt, dt], True, None, True))
    docs.append(("mixed terminators", document(rng, ALL_SIX, 90, terminators=("\n", "\r", "\r\n")), ALL_SIX, True, None, True))
    docs.append(("crlf, blank lines, open end", document(rng, ALL_SIX, 90, terminators=("\r\n",), blank_lines=True,
                                                         last_terminated=False), ALL_SIX, True, None, True))
    docs.append(("no header, all six", document(rng, ALL_SIX, 70, header=False), ALL_SIX, False, None, True))
    return docs


# (name, bytes, dtypes, has_header, (row, column)) -- one per rule, the answers by hand
REFUSALS = [
    ("stray quote", b'a,b\n1,x\n2,y"z\n', [M.INT64, M.UTF8], True, (1, 1)),
    ("byte after closing quote", b'a,b\n1,"x"y\n', [M.INT64, M.UTF8], True, (0, 1)),
    ("space after closing quote", b'a,b\n"1" ,x\n', [M.INT64, M.UTF8], True, (0, 0)),
    ("unterminated quote", b'a,b\n1,x\n2,"y\n3,z\n', [M.INT64, M.UTF8], True, (1, 1)),
    ("too few fields", b"a,b,c\n1,2,3\n4,5\n", [M.INT64] * 3, True, (1, 2)),
    ("too many fields", b"a,b\n1,2\n3,4,5\n", [M.INT64] * 2, True, (1, 2)),
    ("trailing delimiter", b"a,b\n1,2,\n", [M.INT64] * 2, True, (0, 2)),
    ("header too short", b"a\n1,2\n", [M.INT64] * 2, True, (-1, 1)),
    ("header too long", b"a,b,c\n1,2\n", [M.INT64] * 2, True, (-1, 2)),
    ("plus sign", b"a\n1\n+5\n", [M.INT64], True, (1, 0)),
    ("leading space", b"a\n 5\n", [M.INT64], True, (0, 0)),
    ("trailing space in a float", b"a\n5 \n", [M.FLOAT64], True, (0, 0)),
    ("fraction in an integer", b"a,b\n1,1.5\n", [M.INT64] * 2, True, (0, 1)),
    ("open exponent", b"a\n1e\n", [M.FLOAT64], True, (0, 0)),
    ("yes", b"a\ntrue\nyes\n", [M.BOOL], True, (1, 0)),
    ("30 February", b"a\n2023-02-28\n2023-02-30\n", [M.DATE32], True, (1, 0)),
    ("short date", b"a\n2023-2-3\n", [M.DATE32], True, (0, 0)),
    ("year 0000", b"a\n0000-01-01\n", [M.DATE32], True, (0, 0)),
    ("2^31 in Int32", b"a,b\n2147483647,-2147483648\n-2147483649,0\n", [M.INT32] * 2, True, (1, 0)),
    ("2^31 in Int32, positive", b"a\n2147483648\n", [M.INT32], True, (0, 0)),
    ("2^63 in Int64", b"a\n9223372036854775808\n", [M.INT64], True, (0, 0)),
    ("invalid UTF-8", b"a,b\n1,x\n2,\xff\n", [M.INT64, M.UTF8], True, (1, 1)),
    ("truncated UTF-8", b"a,b\n1,\xe6\x97\n", [M.INT64, M.UTF8], True, (0, 1)),
    ("overlong form", b"a\n\xc0\xaf\n", [M.UTF8], True, (0, 0)),
    ("overlong three-byte form", b"a\nok\n\xe0\x80\xaf\n", [M.UTF8], True, (1, 0)),
    ("surrogate", b"a\n\xed\xa0\x80\n", [M.UTF8], True, (0, 0)),
    ("above U+10FFFF", b"a\n\xf4\x90\x80\x80\n", [M.UTF8], True, (0, 0)),
    ("invalid UTF-8 in the header", b"a,\xff\n1,2\n", [M.INT64] * 2, True, (-1, 1)),
    ("escaped quote in a number", b'a\n"1""2"\n', [M.INT64], True, (0, 0)),
    ("lower column wins", b'a,b,c\n1,2,3\nx,2,"3"4\n', [M.INT64] * 3, True, (1, 0)),
]


def two_refusals():
    """A grammar refusal in row 40 and a stray quote in row 9000: the first is reported."""
    lines = ["a,b"] + [f"{i},w{i}" for i in range(10_000)]
    lines[1 + 40] = "4x0,w"
    lines[1 + 9000] = '9000,w"w'
    return "\n".join(lines).encode() + b"\n", [M.INT64, M.UTF8], (40, 0)


# ---- CPU: the model ---------------------------------------------------------------------------------

def test_model_hand_answers_and_pyarrow():
    for name, data, dtypes, header, want, with_arrow in dialect_documents():
        got = M.parse(data, dtypes, header)
        assert not isinstance(got, M.Refused), (name, got)
        if want is not None:
            assert got == want, name
        if with_arrow:
            assert_model_equals_arrow(got, arrow_table(data, dtypes, header), dtypes)


def test_model_refusals():
    for name, data, dtypes, header, want in REFUSALS:
        got = M.parse(data, dtypes, header)
        assert isinstance(got, M.Refused) and (got.row, got.col) == want, (name, got)
    data, dtypes, want = two_refusals()
    got = M.parse(data, dtypes, True)
    assert isinstance(got, M.Refused) and (got.row, got.col) == want


# ---- GPU ---------------------------------------------------------------------------------------------

REFUSED_RE = re.compile(r"csv: row (-?\d+), column (\d+): ")


def device_equals_model(ctx, data, dtypes, has_header=True, model=None, source=None):
    """qeh_scan_csv over `data` against the model: equal columns, or a refusal at the model's place."""
    model = M.parse(data, dtypes, has_header) if model is None else model
    src = data if source is None else source
    if isinstance(model, M.Refused):
        with pytest.raises(qe_hip.QehError) as e:
            ctx.scan_csv(src, schema_of(dtypes), has_header)
        assert e.value.status == abi.QEH_E_UNSUPPORTED, e.value
        m = REFUSED_RE.match(e.value.message)
        assert m and (int(m.group(1)), int(m.group(2))) == (model.row, model.col), (e.value.message, model)
        return None
    cols = ctx.scan_csv(src, schema_of(dtypes), has_header)
    assert len(cols) == len(dtypes)
    for col, dt, (values, valid) in zip(cols, dtypes, model):
        n = len(values)
        nulls = n - sum(valid)
        assert len(col) == n and col.c.offset == 0 and col.c.owned == 1
        assert col.c.null_count == nulls
        mask = col.valid_mask()
        if nulls == 0:
            assert not col.c.validity and mask is None
        else:
            assert mask is not None and mask.tolist() == valid
        if dt == M.UTF8:
            offs = np.zeros(n + 1, np.int32)
            ctx.d2h(offs, col.c.offsets, 4 * (n + 1))
            want = np.concatenate([[0], np.cumsum([len(v) for v in values], dtype=np.int64)]) if n else np.zeros(1, np.int64)
            assert offs.tolist() == want.tolist() and col.c.values_bytes == want[-1]
            assert col.to_bytes() == values
            continue
        got, _ = col.to_numpy()
        if dt == M.FLOAT64:
            assert got.view(np.uint64).tolist() == [f64_bits(v) for v in values]
        elif dt == M.DATE32:
            assert got.astype(np.int64).tolist() == values
        else:
            assert got.tolist() == values
    return cols


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, "4"])
def test_device_equals_model_on_the_dialect(ctx, monkeypatch, chunk):
    if chunk:
        monkeypatch.setenv("QEH_CSV_CHUNK", chunk)
    for name, data, dtypes, header, want, with_arrow in dialect_documents():
        model = M.parse(data, dtypes, header)
        cols = device_equals_model(ctx, data, dtypes, header, model)
        if with_arrow:  # the device equals pyarrow too, where pyarrow reads the dialect alike
            table = arrow_table(data, dtypes, header)
            for col, dt, acol in zip(cols, dtypes, table.columns):
                got = col.to_arrow()
                if dt == M.FLOAT64:
                    assert got.is_valid().to_pylist() == acol.is_valid().to_pylist()
                    a = got.fill_null(0.0).to_numpy(zero_copy_only=False).view(np.uint64)
                    b = acol.combine_chunks().fill_null(0.0).to_numpy(zero_copy_only=False).view(np.uint64)
                    assert a.tolist() == b.tolist(), name
                else:
                    assert got.to_pylist() == acol.to_pylist(), name


@pytest.mark.gpu
def test_hundred_thousand_rows_from_host_and_device_bytes(ctx):
    import torch
    rng = random.Random(5)
    data = document(rng, ALL_SIX, 100_003, terminators=("\n", "\r\n"), last_terminated=False)
    model = M.parse(data, ALL_SIX, True)
    assert len(model[0][0]) == 100_003
    device_equals_model(ctx, data, ALL_SIX, True, model)
    dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).to("cuda:0")
    device_equals_model(ctx, data, ALL_SIX, True, model, source=dev)
    odd = torch.frombuffer(bytearray(b"###" + data), dtype=torch.uint8).to("cuda:0")[3:]  # no 16-B alignment
    device_equals_model(ctx, data, ALL_SIX, True, model, source=odd)


EDGE_BODY = ('1,"a,""b""\r\nc",1.5\r\n2,naïve 日本 😀,-2.5e-3\r"3","""","7"\n\n\r\n4,"",\r\n'
             '5,"é\n\n""","0.1"\r6,x,\n').encode() * 12
EDGE_TYPES = [M.INT32, M.UTF8, M.FLOAT64]


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, "4"])
def test_every_construct_at_every_edge_position(ctx, monkeypatch, chunk):
    """A padding record of 0..70 bytes in front shifts every quote pair, CRLF and multi-byte
    character over every thread, wave (chunk 4: 256 B) and workgroup (1024 B) edge position."""
    if chunk:
        monkeypatch.setenv("QEH_CSV_CHUNK", chunk)
    assert len(EDGE_BODY) > 1100
    want = M.parse(EDGE_BODY, EDGE_TYPES, False)
    assert not isinstance(want, M.Refused) and len(want[0][0]) == 72
    for pad in range(0, 71):
        if pad == 0:
            front, extra = b"", 0
        elif pad == 1:
            front, extra = b"\n", 0  # (one byte holds no three fields: a record without bytes)
        else:
            front, extra = b"," + b"p" * (pad - 2) + b",\n", 1  # the record (NULL, "pp..", NULL) of `pad` bytes
        model = M.parse(front + EDGE_BODY, EDGE_TYPES, False)
        assert [(v[extra:], ok[extra:]) for v, ok in model] == want, pad
        device_equals_model(ctx, front + EDGE_BODY, EDGE_TYPES, False, model)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, "4"])
def test_long_fields_and_one_record_per_width(ctx, monkeypatch, chunk):
    if chunk:
        monkeypatch.setenv("QEH_CSV_CHUNK", chunk)
    big = ('x,"y"\n' * 50_000)  # 300 000 bytes of commas, quotes and terminators inside one quoted field
    data = ('a,b\n1,"' + big.replace('"', '""') + '"\n2,z\n').encode()
    cols = device_equals_model(ctx, data, [M.INT64, M.UTF8])
    assert cols[1].c.values_bytes == len(big) + 1
    # one record of every byte width 1..300 (a single Utf8 column; width 2 also as the empty field "")
    lines = ["w" * n for n in range(1, 301)] + ['""', '"q"', '"' + "é" * 40 + '"']
    device_equals_model(ctx, ("\n".join(lines) + "\n").encode(), [M.UTF8], has_header=False)
    device_equals_model(ctx, "\r\n".join(lines).encode(), [M.UTF8], has_header=False)


@pytest.mark.gpu
def test_numeric_edges(ctx):
    cells = edge_float_cells() + random_reprs(20_000, seed=9)
    data = ("f\n" + "\n".join(cells) + "\n").encode()
    cols = device_equals_model(ctx, data, [M.FLOAT64])
    assert len(cols[0]) == len(cells)
    quoted = ("f,g\n" + "\n".join(f'"{c}",{c}' for c in cells[:3000]) + "\n").encode()
    device_equals_model(ctx, quoted, [M.FLOAT64, M.FLOAT64])
    ints = b"a,b\n-0,007\n-9223372036854775808,2147483647\n9223372036854775807,-2147483648\n" + b"0" * 50 + b"9,-000\n"
    cols = device_equals_model(ctx, ints, [M.INT64, M.INT32])
    assert cols[0].to_numpy()[0].tolist() == [0, -2**63, 2**63 - 1, 9]
    assert cols[1].to_numpy()[0].tolist() == [7, 2**31 - 1, -2**31, 0]


@pytest.mark.gpu
def test_floats_the_device_cannot_decide_are_parsed_on_the_host(ctx):
    halfway = halfway_cells(random.Random(21), 200)
    data = ("f\n" + "\n".join(halfway) + "\n").encode()
    ctx.timing(True)
    ctx.timing_reset()
    try:
        device_equals_model(ctx, data, [M.FLOAT64])
        _, patched = ctx.kernel_time("csv_float_patch")
    finally:
        ctx.timing(False)
    assert 0 < patched <= len(halfway)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk", [None, "4"])
def test_refusals(ctx, monkeypatch, chunk):
    if chunk:
        monkeypatch.setenv("QEH_CSV_CHUNK", chunk)
    ex = QueryExecutor(ctx)
    for name, data, dtypes, header, want in REFUSALS:
        model = M.parse(data, dtypes, header)
        assert (model.row, model.col) == want, name
        device_equals_model(ctx, data, dtypes, header, model)
    data, dtypes, want = two_refusals()
    model = M.parse(data, dtypes, True)
    assert (model.row, model.col) == want
    device_equals_model(ctx, data, dtypes, True, model)
    assert ex.cache_stats()["entries"] >= 0


@pytest.mark.gpu
def test_schema_refusals_and_bad_arguments(ctx):
    for t in (pa.float32(), pa.date64(), pa.timestamp("us")):
        with pytest.raises(qe_hip.QehError) as e:
            ctx.scan_csv(b"a\n1\n", pa.schema([pa.field("a", t)]))
        assert e.value.status == abi.QEH_E_UNSUPPORTED and e.value.message.startswith("csv: schema, column 0")
    with pytest.raises(qe_hip.QehError) as e:
        ctx.scan_csv(b"a\n1\n", pa.schema([pa.field("a", pa.uint32())]))
    assert e.value.status == abi.QEH_E_INVALID
    out, rows = (abi.QehColumn * 1)(), C.c_int64()
    dts = (C.c_int32 * 1)(abi.DT_INT64)
    assert ctx.lib.qeh_scan_csv(ctx.h, None, 4, 0, 1, dts, 1, out, C.byref(rows)) == abi.QEH_E_INVALID
    assert ctx.lib.qeh_scan_csv(ctx.h, b"a\n1\n", 4, 0, 2, dts, 1, out, C.byref(rows)) == abi.QEH_E_INVALID
    assert ctx.lib.qeh_scan_csv(ctx.h, b"a\n1\n", 4, 0, 1, dts, 0, out, C.byref(rows)) == abi.QEH_E_INVALID


# ---- the plan over preloaded CSV sources -----------------------------------------------------------

EMP = pa.schema([("employees.id", pa.int64()), ("employees.name", pa.string()), ("employees.age", pa.int64()),
                 ("employees.salary", pa.int64()), ("employees.dept_id", pa.string())])  # the file holds the text NULL
DEP = pa.schema([("departments.dept_id", pa.string()), ("departments.dept_name", pa.string()),
                 ("departments.location", pa.string()), ("departments.manager", pa.string())])
ON = binop(Column("employees.dept_id", 4), BinaryOp.Equal, Column("departments.dept_id", 5))


class NoBatches(CsvDataSource):
    """The same source with zero host batches: a result can only come from the parsed columns."""

    def scan(self):
        return []


def plans(es, ds):
    join = HashJoin(Scan(es), Scan(ds), JoinType.Inner, ON)
    names = Projection(join, [Column("employees.name", 1), Column("departments.dept_name", 6)],
                       ["employees.name", "departments.dept_name"])
    s = Column("employees.salary", 3)
    grouped = HashAggregate(Filter(HashJoin(Scan(es), Scan(ds), JoinType.Inner, ON),
                                   binop(Column("employees.age", 2), BinaryOp.Greater, lit(25))),
                            [Column("departments.dept_id", 5)], [AggregateExpr(AF.Count, s), AggregateExpr(AF.Sum, s)])
    left = Projection(HashJoin(Scan(es), Scan(ds), JoinType.Left, ON),
                      [Column("employees.name", 1), Column("departments.dept_name", 6)],
                      ["employees.name", "departments.dept_name"])
    return [names, grouped, left]


def rows_of(batches):
    t = pa.Table.from_batches(batches)
    return t.schema.names, sorted(zip(*[t.column(i).to_pylist() for i in range(t.num_columns)]), key=repr)


@pytest.mark.gpu
def test_plan_over_preloaded_csv_sources(ctx):
    ex = QueryExecutor(ctx)
    emp_path, dep_path = os.path.join(GOLD, "employees.csv"), os.path.join(GOLD, "departments.csv")
    es, ds = NoBatches(emp_path, EMP), NoBatches(dep_path, DEP)
    assert es.preload(ctx) and ds.preload(ctx)
    host_e, host_d = CsvDataSource(emp_path, EMP, device_cache=False), CsvDataSource(dep_path, DEP, device_cache=False)
    assert pa.Table.from_batches(host_e.scan()).num_rows == 6
    before = ex.cache_stats()
    for dev_plan, host_plan in zip(plans(es, ds), plans(MemoryDataSource(EMP, host_e.scan()), MemoryDataSource(DEP, host_d.scan()))):
        got, want = rows_of(ex.execute(dev_plan)), rows_of(ex.execute(host_plan))
        assert got == want and len(want[1]) > 0
    after = ex.cache_stats()
    assert after["hits"] - before["hits"] == 6 and after["misses"] == before["misses"]
    names, rows = rows_of(ex.execute(plans(es, ds)[0]))
    assert names == ["employees.name", "departments.dept_name"]
    assert rows == sorted([("Alice", "Engineering"), ("Bob", "Sales"), ("Charlie", "Engineering"), ("Diana", "HR"),
                           ("Eve", "Sales")], key=repr)
    ex.cache_evict(es)
    ex.cache_evict(ds)


@pytest.mark.gpu
def test_refused_file_falls_back_to_the_host_batches(ctx, tmp_path):
    ex = QueryExecutor(ctx)
    path = tmp_path / "employees_spaced.csv"
    text = open(os.path.join(GOLD, "employees.csv")).read().replace("2,Bob,30", "2,Bob, 30")  # pyarrow trims, the device refuses
    path.write_text(text)
    es = CsvDataSource(str(path), EMP)
    ds = CsvDataSource(os.path.join(GOLD, "departments.csv"), DEP)
    entries = ex.cache_stats()["entries"]
    assert es.preload(ctx) is False
    assert ex.cache_stats()["entries"] == entries  # the cache is untouched
    assert ds.preload(ctx) is True
    got = rows_of(ex.execute(plans(es, ds)[1]))
    good = CsvDataSource(os.path.join(GOLD, "employees.csv"), EMP, device_cache=False)
    want = rows_of(ex.execute(plans(MemoryDataSource(EMP, good.scan()), ds)[1]))
    assert got == want and len(want[1]) == 3
    ex.cache_evict(es)
    ex.cache_evict(ds)
