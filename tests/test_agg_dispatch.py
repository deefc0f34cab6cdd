"""The (NTERMS, NACOL, NT) dispatch of the fast aggregate kernels (dispatch_fast, csrc/aggregate.h) at
each of its five launch sites: 0 / 1 / 2 conjunctive compare terms x COUNT only / one / two aggregate
columns, checked exactly against a numpy restatement of the query (small integer values, so every
SUM is exact).  The probe is two slice tiles plus 17 rows: full tiles and a ragged tail for every
site's tile (2048 .. 8192 rows), more than one workgroup.  A three-term predicate leaves the fast
kernels and must still agree.  QEH_NT_LOADS is read once per process, so the NT half is not swept."""
import os
import re

import numpy as np
import pytest

from qe_hip import AggregateFunction as AF
from qe_hip import BinaryOp, binop, col, lit

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "query-engine_amd", "csrc")


def _const(header, name):
    with open(os.path.join(CSRC, header)) as f:
        return int(re.search(r"constexpr int %s = (\d+);" % name, f.read()).group(1))


SLICE_TILE = _const("agg_device.h", "kSliceBlock") * 2 * _const("fast_tile.h", "kFastPairs")  # phase A's rows per tile
N = 2 * SLICE_TILE + 17
N_DIM, GROUPS, KEY0 = 300, 16, -40

# probe columns: 0 x, 1 y (predicate inputs), 2 join key, 3 v (Int64), 4 w (Float64, whole numbers), 5 group key
X, Y, K, V, W, G = range(6)
PREDS = {
    0: None,
    1: binop(col(X), BinaryOp.Greater, lit(49)),
    2: binop(col(X), BinaryOp.Greater, lit(20)) & binop(col(Y), BinaryOp.Less, lit(80)),
    3: (binop(col(X), BinaryOp.Greater, lit(20)) & binop(col(Y), BinaryOp.Less, lit(80)))
       & binop(col(X), BinaryOp.NotEqual, lit(50)),
}
AGGS = {
    0: [(AF.Count, V)],
    1: [(AF.Sum, V), (AF.Count, V), (AF.Max, V)],
    2: [(AF.Sum, V), (AF.Sum, W), (AF.Count, V), (AF.Min, W)],
}


@pytest.fixture(scope="module")
def data():
    r = np.random.default_rng(0xA66)
    cols = [r.integers(0, 100, N), r.integers(0, 100, N),
            r.integers(KEY0 - 10, KEY0 + N_DIM + 10, N),  # misses below and above the build keys
            r.integers(-50, 50, N), r.integers(-50, 50, N).astype(np.float64), r.integers(0, 40, N)]
    cols = [np.ascontiguousarray(c, dtype=c.dtype if c.dtype == np.float64 else np.int64) for c in cols]
    dk = r.permutation(N_DIM).astype(np.int64) + KEY0
    dg = r.integers(0, GROUPS, N_DIM).astype(np.int64) - 5
    sel = {0: np.ones(N, bool), 1: cols[X] > 49, 2: (cols[X] > 20) & (cols[Y] < 80)}
    sel[3] = sel[2] & (cols[X] != 50)
    group_of_key = np.full(N_DIM + 20, np.iinfo(np.int64).min)
    group_of_key[dk - (KEY0 - 10)] = dg
    joined = group_of_key[cols[K] - (KEY0 - 10)]  # the build row's group, INT64_MIN where no build row matches
    return cols, dk, dg, sel, joined


def restate(cols, sel, gid, aggs):
    """Groups (sorted) and aggregates of the selected rows, in the device's output types."""
    keys = np.unique(gid[sel])
    out = []
    for f, c in aggs:
        rows = [cols[c][sel & (gid == k)] for k in keys]
        if f == AF.Count:
            out.append(np.array([len(x) for x in rows], np.int64))
        else:
            fn = {AF.Sum: np.sum, AF.Min: np.min, AF.Max: np.max}[f]
            out.append(np.array([fn(x) for x in rows], cols[c].dtype))
    return keys, out


def check(got_keys, got_aggs, want_keys, want_aggs):
    (gk, gk_valid), = [c.to_numpy() for c in got_keys]
    assert gk_valid is None or gk_valid.all()
    order = np.argsort(gk, kind="stable")
    assert gk.dtype == want_keys.dtype and np.array_equal(gk[order], want_keys)
    for j, (c, want) in enumerate(zip(got_aggs, want_aggs)):
        vals, valid = c.to_numpy()
        assert valid is None or valid.all(), j
        assert vals.dtype == want.dtype and np.array_equal(vals[order], want), (j, vals[order], want)


def counts(ctx, fn):
    ctx.timing(True)
    ctx.timing_reset()
    try:
        out = fn()
        n = {name: ctx.kernel_time(name)[1] for name in ("fused_build", "slice_partition", "slice_probe", "bucket_parts")}
    finally:
        ctx.timing(False)
    return out, n


# site -> environment that forces it, and the timing records that show it ran (the others must be absent)
SITES = {
    "fast": ({}, ()),
    "bucket": ({"QEH_BUCKET_PARTS": "1", "QEH_FORCE_TABLE": "bucket"}, ("bucket_parts",)),
    "slice": ({"QEH_NO_FUSED": "1", "QEH_SLICE_MIN_BYTES": "0"}, ("slice_partition", "slice_probe")),
    "fused": ({"QEH_SLICE_MIN_BYTES": "0"}, ("fused_build", "slice_partition", "slice_probe")),
}


@pytest.mark.gpu
@pytest.mark.parametrize("site,nterms,nacol", [
    (s, t, a) for s in SITES for t in (0, 1, 2, 3) for a in (0, 1, 2)
    if not (s == "bucket" and a == 2)])  # the bucket probe stages one value column: two never reach it
def test_join_sites(ctx, monkeypatch, data, site, nterms, nacol):
    cols, dk, dg, sel, joined = data
    env, ran = SITES[site]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    probe = [ctx.upload(c) for c in cols]
    (gk, ga, g), n = counts(ctx, lambda: ctx.join_filter_aggregate(probe, K, PREDS[nterms], ctx.upload(dk), [ctx.upload(dg)],
                                                                   AGGS[nacol]))
    if nterms == 3:
        ran = ()  # three terms: none of the fast kernels' pipelines may run
    assert all((n[name] >= 1) == (name in ran) for name in n), n
    matched = sel[nterms] & (joined != np.iinfo(np.int64).min)
    wk, wa = restate(cols, matched, joined, AGGS[nacol])
    assert g == len(wk)
    check(gk, ga, wk, wa)


@pytest.mark.gpu
@pytest.mark.parametrize("nacol", [0, 1, 2])
@pytest.mark.parametrize("nterms", [0, 1, 2, 3])
def test_group_by_site(ctx, data, nterms, nacol):
    """Single-key GROUP BY through k_group_agg_fast (256-thread tiles for COUNT alone, 1024-thread
    tiles once the LDS table holds value slots)."""
    cols, _, _, sel, _ = data
    gk, ga, g = ctx.filter_aggregate([ctx.upload(c) for c in cols], PREDS[nterms], [G], AGGS[nacol])
    wk, wa = restate(cols, sel[nterms], cols[G], AGGS[nacol])
    assert g == len(wk)
    check(gk, ga, wk, wa)
