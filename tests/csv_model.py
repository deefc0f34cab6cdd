"""The CSV dialect of the device reader (qeh_scan_csv) in plain Python: the arbiter for the kernels.

Written from the rules below, not from the kernels: one sequential walk over the bytes, `re` for the
cell grammars, float() / int() / datetime.date for the values, bytes.decode for UTF-8.

  Records   ',' delimits, '"' quotes, nothing escapes.  A record ends at \\n, \\r or \\r\\n outside quotes,
            or at the end of the input.  Records without bytes are skipped; a line holding only ""
            is a record with one empty field.  With a header the first record is skipped, but it
            must have the right number of fields (and be well formed).
  Quoting   a field is quoted iff its first byte is '"'.  Inside, "" is one quote; delimiters and
            terminators are data.  After the closing quote comes ',', a terminator or the end.
            Refused: any other byte after a closing quote, a quote inside an unquoted field, a
            quoted field still open at the end of the input.
  Count     every record has exactly n_cols fields.
  NULL      an empty field, quoted or not, of any type.
  Cells     Int32 / Int64  -?[0-9]+ in range.   Bool  true / false, ASCII case-insensitive.
            Float64  -?([0-9]+(\\.[0-9]*)?|\\.[0-9]+)([eE][+-]?[0-9]+)? or nan / inf / infinity with an
            optional '-', any ASCII case: float(cell).   Date32  YYYY-MM-DD, a date of the years
            0001-9999, as days since 1970-01-01.   Utf8  the bytes.  Nothing is trimmed.
  UTF-8     every field's bytes must decode strictly.
  Refusal   the first record that breaks a rule and, within it, the lowest field index (an index past
            the schema counts as n_cols; a record with too few fields breaks the rule at the first
            missing one).  Data rows count from 0; the header is row -1.

parse() returns one (values, valid) pair per column -- NULL slots hold 0 / 0.0 / False / b"" -- or a
Refused."""
import datetime
import re

INT32, INT64, FLOAT64, BOOL, DATE32, UTF8 = "int32", "int64", "float64", "bool", "date32", "utf8"

_INT = re.compile(rb"-?[0-9]+")
_FLOAT = re.compile(rb"-?([0-9]+(\.[0-9]*)?|\.[0-9]+)([eE][+-]?[0-9]+)?")
_SPECIAL = re.compile(rb"-?(nan|inf|infinity)", re.I)
_DATE = re.compile(rb"([0-9]{4})-([0-9]{2})-([0-9]{2})")
_EPOCH = datetime.date(1970, 1, 1)


class Refused:
    def __init__(self, row, col, why):
        self.row, self.col, self.why = row, col, why

    def __repr__(self):
        return f"Refused(row={self.row}, col={self.col}, {self.why})"


class _Broken(Exception):
    pass


def _field(data, pos):
    """The field that starts at pos: (content with "" collapsed, next field's start or None at the
    record's end, position after the record's last byte)."""
    n = len(data)
    if pos < n and data[pos:pos + 1] == b'"':
        i = pos + 1
        while True:
            j = data.find(b'"', i)
            if j < 0:
                raise _Broken("unterminated quote")
            if data[j + 1:j + 2] == b'"':
                i = j + 2
                continue
            break
        raw = data[pos + 1:j]
        after = data[j + 1:j + 2]
        if after == b",":
            nxt = j + 2
        elif after in (b"", b"\n", b"\r"):
            nxt = None
        else:
            raise _Broken("byte after a closing quote")
        return raw.replace(b'""', b'"'), nxt, j + 1
    i = pos
    while i < n and data[i:i + 1] not in (b",", b"\n", b"\r"):
        if data[i:i + 1] == b'"':
            raise _Broken("quote in an unquoted field")
        i += 1
    return data[pos:i], (i + 1 if data[i:i + 1] == b"," else None), i


def cell_value(dtype, cell):
    """The value of a non-empty cell, or _Broken."""
    if dtype in (INT32, INT64):
        if not _INT.fullmatch(cell):
            raise _Broken("not an integer")
        v = int(cell)
        bits = 31 if dtype == INT32 else 63
        if not -(1 << bits) <= v < (1 << bits):
            raise _Broken("integer out of range")
        return v
    if dtype == FLOAT64:
        if not (_FLOAT.fullmatch(cell) or _SPECIAL.fullmatch(cell)):
            raise _Broken("not a float")
        return float(cell.decode("ascii"))
    if dtype == BOOL:
        if cell.lower() not in (b"true", b"false"):
            raise _Broken("not a boolean")
        return cell.lower() == b"true"
    if dtype == DATE32:
        m = _DATE.fullmatch(cell)
        if not m:
            raise _Broken("not YYYY-MM-DD")
        try:
            d = datetime.date(int(m.group(1)), int(m.group(2)), int(m.group(3)))
        except ValueError:
            raise _Broken("no such date")
        return (d - _EPOCH).days
    if dtype == UTF8:
        return cell
    raise ValueError(dtype)


_ZERO = {INT32: 0, INT64: 0, FLOAT64: 0.0, BOOL: False, DATE32: 0, UTF8: b""}


def parse(data, dtypes, has_header=True):
    data = bytes(data)
    n_cols = len(dtypes)
    cols = [([], []) for _ in dtypes]
    pos, n, row = 0, len(data), -1 if has_header else 0
    while True:
        while pos < n and data[pos:pos + 1] in (b"\n", b"\r"):
            pos += 1  # terminators, and the records without bytes between them
        if pos >= n:
            return cols
        c = 0
        cells = []
        while True:
            try:
                cell, nxt, end = _field(data, pos)
                try:
                    cell.decode("utf-8")
                except UnicodeDecodeError:
                    raise _Broken("invalid UTF-8")
                if c >= n_cols:
                    raise _Broken("too many fields")
                cells.append(cell if row < 0 or not cell else cell_value(dtypes[c], cell))
            except _Broken as e:
                return Refused(row, min(c, n_cols), str(e))
            c += 1
            if nxt is None:
                break
            pos = nxt
        if c < n_cols:
            return Refused(row, c, "too few fields")
        if row >= 0:
            for (values, valid), dt, cell in zip(cols, dtypes, cells):
                null = isinstance(cell, bytes) and not cell
                values.append(_ZERO[dt] if null else cell)
                valid.append(not null)
        pos = end
        row += 1
