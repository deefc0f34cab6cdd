"""Window functions in plain Python: the arbiter for the device kernels and for the C oracle.

Written from docs/WINDOW_FUNCTIONS.md and the rules below, not from the oracle or the kernels: no
numpy in the logic, unbounded ints, Python's `sorted` on explicit key tuples, and every function
stated as its definition over the rows of a partition instead of a walk with running counters.

A column is a pair (values, valid-or-None); `valid[i]` false makes row i NULL whatever values[i] holds.

  Order       PARTITION BY keys ascending, then the ORDER BY keys as given; ties by input position.
  NULLs       a NULL key sorts first whatever the direction; NULLs equal each other, both as a
              partition and as peers.
  Float keys  compared and told apart by IEEE totalOrder of their bits: -0.0 and +0.0 are different
              keys, NaNs with different bits differ; a Float32 key keeps its own 32 bits.
  Bool keys   false before true.  Utf8 keys: byte order.  Temporal keys: their physical integers.
  RANK        1 + the partition's rows ordered strictly before the row; DENSE_RANK: 1 + the distinct
              ORDER BY tuples before it; ROW_NUMBER: the row's place in the partition.
  NTILE(n)    n buckets in order, the first size % n of them hold one row more.
  LAG / LEAD  the row `param` places before / after inside the partition; where that leaves the
              partition, the default, or NULL if none is given.
  FIRST_VALUE / LAST_VALUE  the partition's first and last row (whole-partition frame).
  Values      a value result is the argument's own element (its bits unchanged), NULL where the
              source row is NULL.
"""
import struct
from bisect import bisect_left

ROW_NUMBER, RANK, DENSE_RANK, NTILE, LAG, LEAD, FIRST_VALUE, LAST_VALUE = range(8)


def scalar_key(x):
    """One non-NULL key value as a Python object that orders the way the rules say."""
    if isinstance(x, str):
        return x.encode()
    if isinstance(x, bytes):
        return x
    if isinstance(x, float):
        raw = struct.pack("<d", x)
    elif getattr(getattr(x, "dtype", None), "kind", "") == "f":
        raw = x.tobytes()  # a sized float scalar: its own 4 or 8 bytes
    else:
        return int(x)  # integers, temporal integers, bools (False < True)
    sign = 1 << (8 * len(raw) - 1)
    bits = int.from_bytes(raw, "little")
    return 2 * sign - 1 - bits if bits & sign else bits | sign  # totalOrder as an unsigned integer


def _column_keys(col, asc):
    """Per row (0, 0) for NULL, else (1, +-rank of the value among the column's distinct values)."""
    values, valid = col
    ks = [scalar_key(values[i]) if valid is None or valid[i] else None for i in range(len(values))]
    rank = {k: r for r, k in enumerate(sorted({k for k in ks if k is not None}))}
    return [(0, 0) if k is None else (1, rank[k] if asc else -rank[k]) for k in ks]


def row_keys(part, order, ascending, n):
    """Per row the tuple that orders it: PARTITION BY keys, then ORDER BY keys with their directions."""
    cols = [_column_keys(c, True) for c in part] + [_column_keys(c, a) for c, a in zip(order, ascending)]
    assert all(len(c) == n for c in cols)
    return [tuple(c[i] for c in cols) for i in range(n)]


def sorted_rows(part, order, ascending, n):
    """The input rows in window order."""
    key = row_keys(part, order, ascending, n)
    return sorted(range(n), key=lambda i: (key[i], i))


def ntile(place, size, n):
    """Bucket (1-based) of the row at `place` (0-based) in a partition of `size` rows."""
    q, r = divmod(size, n)
    big = r * (q + 1)  # rows in the r buckets of q + 1
    return place // (q + 1) + 1 if place < big else r + (place - big) // q + 1


def window(func, part, order, ascending, arg=None, param=0, default=None, n=None):
    """(values, valid) per input row.  Ranking functions give ints, all valid; value functions give
    the argument's own elements (or `default`), None where the result is NULL."""
    if n is None:
        n = len((list(part) + list(order) + [arg])[0][0])
    if func == NTILE and param < 1:
        raise ValueError("NTILE needs a bucket count >= 1")
    if func in (LAG, LEAD) and param < 0:
        raise ValueError("LAG/LEAD offset must be >= 0")
    key = row_keys(part, order, ascending, n)
    partitions = {}
    for row in sorted(range(n), key=lambda i: (key[i], i)):
        partitions.setdefault(key[row][:len(part)], []).append(row)
    out, ok = [None] * n, [True] * n
    for rows in partitions.values():
        size = len(rows)
        okeys = [key[r][len(part):] for r in rows]  # non-decreasing
        distinct = sorted(set(okeys))
        for place, row in enumerate(rows):
            if func == ROW_NUMBER:
                out[row] = place + 1
            elif func == RANK:
                out[row] = 1 + bisect_left(okeys, okeys[place])
            elif func == DENSE_RANK:
                out[row] = 1 + bisect_left(distinct, okeys[place])
            elif func == NTILE:
                out[row] = ntile(place, size, param)
            else:
                at = {LAG: place - param, LEAD: place + param, FIRST_VALUE: 0, LAST_VALUE: size - 1}[func]
                if 0 <= at < size:
                    src = rows[at]
                    ok[row] = bool(arg[1] is None or arg[1][src])
                    out[row] = arg[0][src] if ok[row] else None
                else:
                    ok[row], out[row] = default is not None, default
    return out, ok
