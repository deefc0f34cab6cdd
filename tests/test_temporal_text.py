"""tests/temporal_text.py (the checker of the device's date / timestamp text) against hand-written
strings: the epoch, the day before it, a leap day, both ends of the year range, the Date64 "NULL"
quirk and the three fraction widths."""
import pytest

import temporal_text as tt


def test_date32_known_answers():
    assert tt.date_text(0) == "1970-01-01"
    assert tt.date_text(-1) == "1969-12-31"
    assert tt.date_text(11016) == "2000-02-29"
    assert tt.date_text(-719528) == "0000-01-01"
    assert tt.date_text(2932896) == "9999-12-31"
    assert tt.date_text(-719528 + 59) == "0000-02-29"  # year 0 is a leap year
    assert tt.date_text(-719162) == "0001-01-01"


def test_date64_known_answers_and_null_quirk():
    assert tt.date64_text(-1) == "NULL"
    assert tt.date64_text(-1000) == "1969-12-31"
    assert tt.date64_text(-1001) == "NULL"
    assert tt.date64_text(0) == "1970-01-01"
    assert tt.date64_text(999) == "1970-01-01"
    assert tt.date64_text(86400000) == "1970-01-02"
    assert tt.date64_text(-86400000) == "1969-12-31"
    assert tt.date64_text(-86401000) == "1969-12-30"


def test_timestamp_known_answers():
    assert tt.timestamp_text(1, "ts_us") == "1970-01-01T00:00:00.000001"
    assert tt.timestamp_text(-1, "ts_us") == "1969-12-31T23:59:59.999999"
    assert tt.timestamp_text(1500, "ts_ms") == "1970-01-01T00:00:01.500"
    assert tt.timestamp_text(0, "ts_s") == "1970-01-01T00:00:00"
    assert tt.timestamp_text(1500000, "ts_us") == "1970-01-01T00:00:01.500"      # a multiple of 1e6 ns: 3 digits
    assert tt.timestamp_text(1, "ts_ns") == "1970-01-01T00:00:00.000000001"
    assert tt.timestamp_text(1000, "ts_ns") == "1970-01-01T00:00:00.000001"
    assert tt.timestamp_text(951782400 + 86399, "ts_s") == "2000-02-29T23:59:59"


def test_years_outside_the_range_raise():
    for days in (-719529, 2932897):
        with pytest.raises(ValueError):
            tt.date_text(days)
    with pytest.raises(ValueError):
        tt.timestamp_text((2932897) * 86400, "ts_s")


def test_cells_and_framing():
    assert tt.cell_text("date32", None) is None
    assert tt.cell_text("date64", -1) == b"NULL"
    assert tt.cell_text("int64", 7) == b"7"
    rows = tt.encode_rows([("date32", [0, None]), ("ts_ms", [1500, 0])])
    assert rows[0] == (b"D" + (4 + 2 + 4 + 10 + 4 + 23).to_bytes(4, "big") + b"\x00\x02" + b"\x00\x00\x00\x0a1970-01-01" +
                       b"\x00\x00\x00\x171970-01-01T00:00:01.500")
    assert rows[1] == (b"D" + (4 + 2 + 4 + 4 + 19).to_bytes(4, "big") + b"\x00\x02" + b"\xff\xff\xff\xff" +
                       b"\x00\x00\x00\x131970-01-01T00:00:00")
