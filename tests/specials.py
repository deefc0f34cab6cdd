"""Float special values and bit-exact comparison helpers (test_float_specials.py).

Everything here is NumPy on integer views of the float bits: nothing goes through the oracle, the
device library or qe_hip.device.order_keys, so the helpers can check all three."""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import numpy as np

TILE = 2048  # rows of one streaming tile: 256 lanes x 8 rows, lane rows at base + j*128 + {0,1}

# +-0, +-min subnormal, +-min normal, +-1, +-max finite, +-inf, then five quiet NaNs: the default NaN
# of either sign, payload 1, and the all-ones payload of either sign (order keys INT64_MAX / INT64_MIN)
_F64_BITS = [
    0x0000000000000000, 0x8000000000000000, 0x0000000000000001, 0x8000000000000001,
    0x0010000000000000, 0x8010000000000000, 0x3FF0000000000000, 0xBFF0000000000000,
    0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF, 0x7FF0000000000000, 0xFFF0000000000000,
    0x7FF8000000000000, 0xFFF8000000000000, 0x7FF8000000000001, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF,
]
_F32_BITS = [
    0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00800000, 0x80800000, 0x3F800000, 0xBF800000,
    0x7F7FFFFF, 0xFF7FFFFF, 0x7F800000, 0xFF800000,
    0x7FC00000, 0xFFC00000, 0x7FC00001, 0x7FFFFFFF, 0xFFFFFFFF,
]
F64_SPECIALS = np.array(_F64_BITS, np.uint64).view(np.float64)
F32_SPECIALS = np.array(_F32_BITS, np.uint32).view(np.float32)
F64_SPECIALS.setflags(write=False)
F32_SPECIALS.setflags(write=False)


def f64(bits: int) -> np.float64:
    return np.array([bits], np.uint64).view(np.float64)[0]


def f32(bits: int) -> np.float32:
    return np.array([bits], np.uint32).view(np.float32)[0]


def specials_of(dtype) -> np.ndarray:
    return F32_SPECIALS if np.dtype(dtype) == np.float32 else F64_SPECIALS


def bits_of(a: np.ndarray) -> np.ndarray:
    """The values' bit patterns as same-width signed integers (integers and bools unchanged)."""
    a = np.asarray(a)
    if a.dtype.kind == "f":
        return a.view(np.int64 if a.dtype.itemsize == 8 else np.int32)
    return a


def total_key(a: np.ndarray) -> np.ndarray:
    """IEEE totalOrder as a signed Int64 order: b ^ ((b >> 63) & 0x7FFF...) on the Float64 bits
    (Float32 widened first, which keeps sign and payload of a quiet NaN); integers as Int64."""
    a = np.asarray(a)
    if a.dtype.kind != "f":
        return a.astype(np.int64)
    b = a.astype(np.float64).view(np.int64)
    return b ^ ((b >> np.int64(63)) & np.int64(0x7FFFFFFFFFFFFFFF))


def _valid(col) -> np.ndarray:
    vals, valid = col
    return np.ones(len(vals), bool) if valid is None else np.asarray(valid, bool)


def assert_bits_equal(got, want, what: str = "", isnan_only: bool = False) -> None:
    """(values, validity-or-None) pairs: same dtype, same validity, identical bits on valid rows.
    isnan_only: a row where either side is NaN need only be NaN on both."""
    gv, wv = np.asarray(got[0]), np.asarray(want[0])
    assert gv.dtype == wv.dtype, f"{what}: dtype {gv.dtype} != {wv.dtype}"
    assert len(gv) == len(wv), f"{what}: length {len(gv)} != {len(wv)}"
    gm, wm = _valid(got), _valid(want)
    assert np.array_equal(gm, wm), f"{what}: validity differs at rows {np.flatnonzero(gm != wm)[:8]}"
    gb, wb = bits_of(gv), bits_of(wv)
    bad = wm & (gb != wb)
    if isnan_only and gv.dtype.kind == "f":
        bad &= ~(np.isnan(gv) & np.isnan(wv))
    if bad.any():
        i = int(np.flatnonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} rows differ; first at {i}: "
                             f"{gv[i]!r} ({int(gb[i]) & (2 ** (8 * gb.itemsize) - 1):#x}) != "
                             f"{wv[i]!r} ({int(wb[i]) & (2 ** (8 * wb.itemsize) - 1):#x})")


def group_order(keys: Sequence[Tuple[np.ndarray, Optional[np.ndarray]]]) -> np.ndarray:
    """Row order by (is_valid, total_key or int value) of each key column, first column most
    significant: -0.0, 0.0 and every NaN pattern are distinct, ordered keys; NULL sorts first."""
    cols = []
    for vals, valid in reversed(list(keys)):
        m = _valid((vals, valid))
        cols.append(np.where(m, total_key(vals), 0))
        cols.append(m)
    return np.lexsort(cols) if cols else np.zeros(1, np.int64)


def assert_grouped_bits_equal(gk, ga, wk, wa, isnan_only: Sequence[int] = (), what: str = "") -> None:
    """Grouped output, any group order: both sides sorted by group_order of their keys, then keys
    and aggregates compared by bits.  Aggregate columns listed in isnan_only (generated NaNs, or a
    NaN carried through a sum) need only be NaN where the other side is."""
    assert len(gk) == len(wk) and len(ga) == len(wa), f"{what}: column counts differ"
    n_got = len((list(gk) + list(ga))[0][0])
    n_want = len((list(wk) + list(wa))[0][0])
    assert n_got == n_want, f"{what}: {n_got} groups != {n_want}"
    go = group_order(gk)[:n_got] if gk else np.arange(n_got)
    wo = group_order(wk)[:n_want] if wk else np.arange(n_want)

    def take(col, order):
        return np.asarray(col[0])[order], _valid(col)[order]
    for j, (g, w) in enumerate(zip(gk, wk)):
        assert_bits_equal(take(g, go), take(w, wo), f"{what} key {j}")
    for j, (g, w) in enumerate(zip(ga, wa)):
        assert_bits_equal(take(g, go), take(w, wo), f"{what} agg {j}", isnan_only=j in isnan_only)


def exact_summable(rng: np.random.Generator, n: int) -> np.ndarray:
    """Float64 k * 2**-10 with integer |k| < 2**20.  For n <= 2**20 every partial sum, in any
    order, is a multiple of 2**-10 below 2**30 in magnitude: at most 50 significant bits, so exact."""
    assert n <= 2 ** 20
    return rng.integers(-(2 ** 20) + 1, 2 ** 20, n).astype(np.float64) * 2.0 ** -10


def special_positions(n: int, rng: np.random.Generator, every: int) -> np.ndarray:
    """Rows with_specials overwrites: the first lane pair, the last row, both sides of every tile
    boundary, and one row in each run of `every`."""
    forced = [0, 1, n - 1]
    for t in range(TILE, n, TILE):
        forced += [t - 1, t]
    scattered = np.arange(0, n, every) + rng.integers(0, every, len(range(0, n, every)))
    pos = np.unique(np.concatenate([np.array(forced, np.int64), scattered]))
    return pos[(pos >= 0) & (pos < n)]


def with_specials(base: np.ndarray, specials: np.ndarray, rng: np.random.Generator, every: int = 4) -> np.ndarray:
    """A copy of `base` with a deterministic scattered subset of rows (special_positions)
    overwritten by the specials, each of them equally often (several times once there are a few
    dozen positions), in shuffled order."""
    out = np.array(base, copy=True)
    pos = special_positions(len(out), rng, every)
    fill = np.asarray(specials)[np.arange(len(pos)) % len(specials)]
    rng.shuffle(fill)
    out[pos] = fill.astype(out.dtype)
    return out
