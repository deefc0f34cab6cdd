"""ORDER BY ... LIMIT k on the device: qeh_sort_indices_limit (MSD radix select on the first key,
ordered compaction of the candidates, the full stable sort over them) and the Limit(Sort) fusion of
the plan executor.

Expected values are the CPU oracle's stable sort permutation cut to k rows (Utf8 keys through
Python-computed dictionary codes, as test_utf8_keys.py does); every comparison is exact.  The GPU
tests put QEH_TOPK_MIN_ROWS at 0 so that the select path, not the small-input fallback, answers."""
import os
import re

import numpy as np
import pyarrow as pa
import pytest

import oracle_bind as ob
import qe_hip
from qe_hip import Limit, MemoryDataSource, QueryExecutor, Scan, Sort, abi
from qe_hip.expr import Column

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 100_003  # not a multiple of any tile
DIGIT_BITS = 11  # csrc/k_topk.hip kTkBits
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max


# ---- CPU: the boundary ------------------------------------------------------------------------

def test_prototype_is_declared_exported_and_bound():
    src = open(os.path.join(ROOT, "include", "qeh.h")).read()
    assert "#define QEH_ABI_VERSION 1" in src  # additive change
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"^\s*int\s+qeh_sort_indices_limit\s*\(([^)]*)\)\s*;", code, flags=re.M)
    assert m, "qeh_sort_indices_limit is not declared in include/qeh.h"
    assert len(m.group(1).split(",")) == 6 and "int64_t limit" in m.group(1)
    assert "qeh_sort_indices_limit" in abi.SIGNATURES
    restype, argtypes = abi.SIGNATURES["qeh_sort_indices_limit"]
    assert len(argtypes) == 6
    assert hasattr(qe_hip.load(), "qeh_sort_indices_limit")
    assert hasattr(qe_hip.Context, "sort_indices_limit")


# ---- helpers ------------------------------------------------------------------------------------

@pytest.fixture(autouse=True)
def select_path(monkeypatch):
    monkeypatch.setenv("QEH_TOPK_MIN_ROWS", "0")


def topk(ctx, cols, asc, k, offset=0):
    """cols: (values, valid-or-None) pairs, values an ndarray or a list of bytes / None (Utf8)."""
    dev = [ctx.upload(v, m) if isinstance(v, list) else ctx.upload(v, m, offset=offset) for v, m in cols]
    return ctx.sort_indices_limit(dev, asc, k).to_numpy()[0]


def host(v, m):
    if isinstance(v, list):  # Utf8: the oracle sorts the Python-computed dictionary codes
        dic = {s: i for i, s in enumerate(sorted({s for s in v if s is not None}))}
        codes = np.array([0 if s is None else dic[s] for s in v], np.int32)
        valid = np.array([s is not None for s in v], bool)
        return ob.HostCol(codes, None if valid.all() else valid)
    return ob.HostCol(v, m)


def want_perm(cols, asc):
    return ob.sort_indices([host(v, m) for v, m in cols], asc)


def check(ctx, cols, asc, k, offset=0, want=None):
    want = want_perm(cols, asc) if want is None else want
    got = topk(ctx, cols, asc, k, offset)
    assert len(got) == min(k, len(want))
    assert np.array_equal(got, want[:k])
    return got


class Timed:
    """ctx.kernel_time launch counts of the calls made inside the block."""

    def __init__(self, ctx):
        self.ctx = ctx

    def __enter__(self):
        self.ctx.timing(True)
        self.ctx.timing_reset()
        return self

    def launches(self, name):
        return self.ctx.kernel_time(name)[1]

    def __exit__(self, *exc):
        self.ctx.timing(False)


# ---- single key ---------------------------------------------------------------------------------

def key_values(dtype, r):
    if dtype == "int32":
        return r.integers(-(2 ** 31), 2 ** 31, N).astype(np.int32)
    if dtype == "int64":
        return r.integers(-(2 ** 50), 2 ** 50, N).astype(np.int64)
    if dtype == "float32":
        return (r.standard_normal(N) * 1e3).astype(np.float32)
    if dtype == "float64":
        v = r.standard_normal(N) * 1e6
        v[r.integers(0, N, 40)] = np.nan
        v[r.integers(0, N, 40)] = -0.0
        v[r.integers(0, N, 40)] = 0.0
        v[r.integers(0, N, 20)] = np.inf
        v[r.integers(0, N, 20)] = -np.inf
        v[7] = -np.nan
        return v
    pool = [b"k%07d" % i for i in r.integers(0, 10 ** 7, 5000)] + [b"", b"\x80", b"a\x00", b"a"]
    return [pool[i] for i in r.integers(0, len(pool), N)]


_single = {}


def single_case(dtype, nulls):
    """The key column and its two oracle permutations, computed once per (dtype, nulls)."""
    if (dtype, nulls) not in _single:
        r = np.random.default_rng(sum((dtype + nulls).encode()))
        v = key_values(dtype, r)
        m = None
        if nulls == "5pct":
            m = r.random(N) >= 0.05
        elif nulls == "3rows":
            m = np.ones(N, bool)
            m[[0, N // 2, N - 1]] = False
        if isinstance(v, list) and m is not None:
            v = [s if ok else None for s, ok in zip(v, m)]
            m = None
        cols = [(v, m)]
        _single[(dtype, nulls)] = (cols, {True: want_perm(cols, [True]), False: want_perm(cols, [False])})
    return _single[(dtype, nulls)]


@pytest.mark.gpu
@pytest.mark.parametrize("k", [0, 1, 7, 1000, N - 1, N, N + 5])
@pytest.mark.parametrize("nulls", ["none", "5pct", "3rows"])
@pytest.mark.parametrize("asc", [True, False])
@pytest.mark.parametrize("dtype", ["int32", "int64", "float32", "float64", "utf8"])
def test_single_key(ctx, dtype, asc, nulls, k):
    cols, want = single_case(dtype, nulls)
    check(ctx, cols, [asc], k, want=want[asc])


# ---- ties ---------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("step", [1, 2 ** 20])
@pytest.mark.parametrize("asc", [True, False])
def test_ties_at_the_threshold_keep_the_lowest_row_ids(ctx, asc, step):
    """40 distinct keys: in [0, 40) (one radix pass sorts them: the full sort answers) and the same
    keys 2^20 apart (the select path answers)."""
    v = np.random.default_rng(3).integers(0, 40, N).astype(np.int64) * step
    with Timed(ctx) as t:
        got = check(ctx, [(v, None)], [asc], 1000)
        assert (t.launches("topk_select") > 0) == (step > 1)
    last = v[got[-1]]  # the threshold value: ~2500 rows carry it, the lowest row ids among them win
    tied = got[v[got] == last]
    assert np.array_equal(tied, np.flatnonzero(v == last)[:len(tied)])


@pytest.mark.gpu
def test_all_keys_equal_falls_back_to_the_full_sort(ctx):
    v = np.full(N, 42, np.int64)
    with Timed(ctx) as t:
        got = check(ctx, [(v, None)], [True], 10)
        assert t.launches("radix_pass") > 0  # mass ties at the threshold: the full sort, cut to 10
    assert np.array_equal(got, np.arange(10))


# ---- key widths ---------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("asc", [True, False])
def test_full_range_int64(ctx, asc):
    v = np.random.default_rng(4).integers(I64_MIN, I64_MAX, N, dtype=np.int64, endpoint=True)
    v[N // 3], v[2 * N // 3] = I64_MIN, I64_MAX
    check(ctx, [(v, None)], [asc], 100)


@pytest.mark.gpu
@pytest.mark.parametrize("asc", [True, False])
def test_every_select_pass_runs(ctx, asc):
    """A 64-bit range whose first 1000 rows end inside a cluster of two adjacent values holding a
    tenth of the rows: the chosen bin stays above the early-stop size until the last digit splits
    the two values, so all ceil(64 / 11) passes run."""
    r = np.random.default_rng(5)
    v = r.integers(I64_MIN // 2, I64_MAX, N, dtype=np.int64)
    c = r.random(N)
    v[c < 0.1] = I64_MIN + 3
    v[c < 0.05] = I64_MIN + 2
    v[11], v[N - 7] = I64_MIN, I64_MAX
    if not asc:
        v = -1 - v  # the mirror image: the cluster just below INT64_MAX
    with Timed(ctx) as t:
        check(ctx, [(v, None)], [asc], 1000)
        assert t.launches("topk_select") > 0


@pytest.mark.gpu
@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("values", [2, 100, 2 ** DIGIT_BITS - 1, 2 ** DIGIT_BITS, 2 ** DIGIT_BITS + 1])
def test_ranges_around_one_digit(ctx, values, nulls):
    """Ranges of one digit, and of exactly 2^b - 1, 2^b and 2^b + 1 codes (the pass count's boundary; a
    nullable key has one more code than values).  A tenth of the rows sit on the two smallest values
    (or the NULLs and the smallest), so the walk goes on to the last digit wherever there are two.
    One key of at most 7 bits is left to the full sort, which needs one radix pass for it."""
    r = np.random.default_rng(values)
    v = r.integers(0, values, N).astype(np.int64)
    c = r.random(N)
    v[c < 0.1] = 1
    v[c < 0.05] = 0
    v[5], v[N - 5] = 0, values - 1  # the whole range is present
    m = (r.random(N) >= 0.04) if nulls else None
    for asc in (True, False):
        check(ctx, [(v if asc else values - 1 - v, m)], [asc], 1500)


# ---- placement ----------------------------------------------------------------------------------

@pytest.mark.gpu
def test_smallest_rows_in_the_last_tile(ctx):
    v = np.random.default_rng(6).integers(10 ** 6, 10 ** 9, N).astype(np.int64)
    v[N - 300:] = np.random.default_rng(7).integers(0, 1000, 300)
    got = check(ctx, [(v, None)], [True], 300)
    assert got.min() >= N - 300


@pytest.mark.gpu
def test_smallest_rows_one_per_tile(ctx):
    v = np.random.default_rng(8).integers(10 ** 6, 10 ** 9, N).astype(np.int64)
    rows = np.arange(0, N, 1024)  # one per 1024 rows: every tile of every kernel holds some
    v[rows] = np.random.default_rng(9).integers(0, 50, len(rows))
    got = check(ctx, [(v, None)], [True], len(rows))
    assert np.array_equal(np.sort(got), rows)


@pytest.mark.gpu
@pytest.mark.parametrize("asc", [True, False])
def test_one_hot_value(ctx, asc):
    """99.9 % of the rows share one large value: whole waves land on one histogram bin."""
    r = np.random.default_rng(10)
    v = np.full(N, 2 ** 40, np.int64)
    rare = r.random(N) < 0.001
    v[rare] = r.integers(0, 2 ** 41, int(rare.sum()))
    check(ctx, [(v, None)], [asc], 30)


# ---- several keys, offsets ----------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("shape", ["pair", "pair_nullable", "three"])
def test_later_keys_decide_the_prefix(ctx, shape):
    """A low-cardinality first key: the prefix ends inside one of its values, so the later keys (and
    then the input position) order the rows that are kept.  `pair`: two non-null keys, the shape
    sort_perm_pair takes."""
    r = np.random.default_rng(12)
    a = r.integers(0, 40, N).astype(np.int64)
    b = r.integers(-50, 50, N).astype(np.int32)
    c = r.standard_normal(N)
    if shape == "pair":
        cols, asc = [(a, None), (c, None)], [True, False]
    elif shape == "pair_nullable":
        cols, asc = [(a, r.random(N) >= 0.02), (b, r.random(N) >= 0.1)], [False, True]
    else:
        cols, asc = [(a, None), (b, r.random(N) >= 0.1), (c, None)], [True, False, True]
    with Timed(ctx) as t:
        check(ctx, cols, asc, 2000)
        assert t.launches("topk_select") > 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", [np.int64, np.int32, np.float64])
def test_column_offset_and_unaligned_validity(ctx, dtype):
    r = np.random.default_rng(13)
    v = r.integers(-10 ** 6, 10 ** 6, N).astype(dtype)
    m = r.random(N) >= 0.03
    check(ctx, [(v, m)], [True], 500, offset=3)
    check(ctx, [(v, None)], [False], 500, offset=3)


# ---- path, errors -------------------------------------------------------------------------------

@pytest.mark.gpu
def test_select_path_runs_and_switches_off(ctx, monkeypatch):
    v = np.random.default_rng(14).integers(-10 ** 9, 10 ** 9, N).astype(np.int64)
    with Timed(ctx) as t:
        a = check(ctx, [(v, None)], [True], 100)
        assert t.launches("topk_select") > 0
    monkeypatch.setenv("QEH_NO_TOPK", "1")
    with Timed(ctx) as t:
        b = check(ctx, [(v, None)], [True], 100)
        assert t.launches("topk_select") == 0
    assert np.array_equal(a, b)


@pytest.mark.gpu
def test_errors(ctx):
    a, b = ctx.upload(np.arange(10, dtype=np.int64)), ctx.upload(np.arange(9, dtype=np.int64))
    with pytest.raises(qe_hip.QehError) as e:
        ctx.sort_indices_limit([a], [True], -1)
    assert e.value.status == abi.QEH_E_INVALID
    with pytest.raises(qe_hip.QehError) as full:
        ctx.sort_indices([a, b], [True, True])
    with pytest.raises(qe_hip.QehError) as e:
        ctx.sort_indices_limit([a, b], [True, True], 3)
    assert (e.value.status, str(e.value)) == (full.value.status, str(full.value))


# ---- plan ---------------------------------------------------------------------------------------

def plan_table(n):
    r = np.random.default_rng(15)
    k = pa.array(r.integers(0, 40, n), pa.int64(), mask=r.random(n) < 0.05)
    w = pa.array(r.random(n))
    s = pa.array([None if x < 0.1 else "p%d" % i for i, x in enumerate(r.random(n))], pa.string())
    return pa.table({"t.k": k, "t.w": w, "t.s": s})


def source(t, chunks=1):
    batches = t.to_batches()
    if chunks > 1 and t.num_rows:
        step = max(1, t.num_rows // chunks)
        batches = [t.slice(i, step).to_batches()[0] for i in range(0, t.num_rows, step)]
    return MemoryDataSource(t.schema, batches)


def sort_plan(t, chunks=1):
    return Sort(Scan(source(t, chunks)), [Column("t.k", 0), Column("t.w", 1)], [True, False])


@pytest.mark.gpu
def test_plan_limit_over_sort(ctx, monkeypatch):
    t = plan_table(N)
    qx = QueryExecutor(ctx)
    plan = Limit(sort_plan(t, 5), 100, 1000)
    with Timed(ctx) as tm:
        out = qx.execute(plan)
        assert tm.launches("topk_select") > 0
    got = pa.Table.from_batches(out)
    k = t.column(0).combine_chunks()
    perm = ob.sort_indices([ob.HostCol(np.asarray(k.fill_null(0)), ~np.asarray(k.is_null())),
                            ob.HostCol(np.asarray(t.column(1)))], [True, False])
    assert got.schema.names == t.schema.names
    assert got.to_pylist() == t.take(pa.array(perm[100:1100])).to_pylist()
    monkeypatch.setenv("QEH_NO_FUSION", "1")
    assert pa.Table.from_batches(qx.execute(plan)).to_pylist() == got.to_pylist()


@pytest.mark.gpu
@pytest.mark.parametrize("quirk", ["fetch_zero", "skip_past_end", "empty_source", "skip_zero"])
def test_plan_quirks_match_the_unfused_path(ctx, monkeypatch, quirk):
    t = plan_table(0 if quirk == "empty_source" else 3000)
    skip, fetch = {"fetch_zero": (5, 0), "skip_past_end": (10 ** 8, 5), "empty_source": (0, 10),
                   "skip_zero": (0, 17)}[quirk]
    qx = QueryExecutor(ctx)
    plan = Limit(sort_plan(t), skip, fetch)
    fused = qx.execute(plan)
    monkeypatch.setenv("QEH_NO_FUSION", "1")
    unfused = qx.execute(plan)
    assert len(fused) == len(unfused)  # the batch count, "no batches" included
    for a, b in zip(fused, unfused):
        assert a.schema == b.schema and a.to_pylist() == b.to_pylist()
