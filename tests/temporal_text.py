"""CPU restatement of the text the reference's pgwire front end gives Date32, Date64 and Timestamp
cells (crates/query-pgwire/src/result.rs:146-172).  TEST INFRASTRUCTURE ONLY: the checker of
qeh_encode_pg_datarows' temporal cells; rows are framed by oracle/pg_text.py's data_row.

Built on datetime.date.fromordinal, not on the civil-from-days arithmetic the kernel uses.
  Date32     NaiveDate::from_num_days_from_ce_opt(days + 719163).to_string(): YYYY-MM-DD.
  Date64     secs = ms / 1000 (truncating), nsecs = ((ms % 1000) * 1_000_000) as u32; a negative
             remainder wraps past 2e9, DateTime::from_timestamp is None and the cell is the text
             "NULL"; otherwise the date of floor(secs / 86400).
  Timestamp  arrow-cast 53.4.1's array_value_to_string = chrono's NaiveDateTime Debug:
             YYYY-MM-DDTHH:MM:SS, then the fraction only when non-zero, in 3, 6 or 9 digits.
Neither arrow-cast nor chrono is available here, so this restates their published behaviour
(parity unpinned against the crates themselves).  Years outside 0000-9999 raise ValueError: chrono
switches to a signed five-digit form there, which the device declines to render.
"""
from __future__ import annotations

import datetime
import os
import sys
from typing import List, Optional, Sequence, Tuple

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import pg_text  # noqa: E402

DAYS_CE_1970 = 719163            # datetime.date(1970, 1, 1).toordinal()
DAYS_400Y = 146097               # the proleptic Gregorian calendar repeats every 400 years
UNIT_PER_SEC = {"ts_s": 1, "ts_ms": 10 ** 3, "ts_us": 10 ** 6, "ts_ns": 10 ** 9}
TEMPORAL = ("date32", "date64") + tuple(UNIT_PER_SEC)


def date_text(days: int) -> str:
    """YYYY-MM-DD of `days` since 1970-01-01."""
    o = int(days) + DAYS_CE_1970
    shift = 0
    if o < 1:  # year 0000 lies before datetime.MINYEAR: read it 400 years later
        o += DAYS_400Y
        shift = 400
    if o < 1 or o > datetime.date.max.toordinal():
        raise ValueError("year outside 0000-9999")
    d = datetime.date.fromordinal(o)
    if d.year < shift:
        raise ValueError("year outside 0000-9999")
    return f"{d.year - shift:04d}-{d.month:02d}-{d.day:02d}"


def date64_text(ms: int) -> str:
    ms = int(ms)
    secs = abs(ms) // 1000 * (1 if ms >= 0 else -1)  # Rust's `/` truncates
    if ms - secs * 1000 < 0:                         # Rust's `%` keeps the sign: the u32 cast wraps
        return "NULL"
    return date_text(secs // 86400)


def timestamp_text(v: int, unit: str) -> str:
    per = UNIT_PER_SEC[unit]
    secs, rem = divmod(int(v), per)  # floor: the fraction is never negative
    nanos = rem * (10 ** 9 // per)
    days, sod = divmod(secs, 86400)
    t = (datetime.datetime(2000, 1, 1) + datetime.timedelta(seconds=sod)).time()
    s = f"{date_text(days)}T{t.hour:02d}:{t.minute:02d}:{t.second:02d}"
    if nanos == 0:
        return s
    if nanos % 10 ** 6 == 0:
        return s + f".{nanos // 10 ** 6:03d}"
    if nanos % 10 ** 3 == 0:
        return s + f".{nanos // 10 ** 3:06d}"
    return s + f".{nanos:09d}"


def cell_text(dtype: str, value) -> Optional[bytes]:
    if value is None:
        return None
    if dtype == "date32":
        return date_text(value).encode()
    if dtype == "date64":
        return date64_text(value).encode()
    if dtype in UNIT_PER_SEC:
        return timestamp_text(value, dtype).encode()
    return pg_text.cell_text(dtype, value)


def encode_rows(columns: Sequence[Tuple[str, list]]) -> List[bytes]:
    """columns: (dtype name, python values with None for NULL) -> one DataRow per row."""
    n = len(columns[0][1]) if columns else 0
    return [pg_text.data_row([cell_text(dt, vals[i]) for dt, vals in columns]) for i in range(n)]
