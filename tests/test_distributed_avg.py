"""Distributed AVG and global aggregates: qeh_avg_finalize (csrc/k_avg_final.hip), the SUM + COUNT
rewrite of AVG in every partial/final plan of qe_hip/distributed.py (expand_avg) and
DistributedExecutor.aggregate.  The multi-process cases run tests/dist_agg_worker.py: ranks share
GPU 0 over gloo, and every float input is exactly summable, so every comparison is exact."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest

import qe_hip
from qe_hip import AggregateFunction as AF, abi

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def launch(mode, world, timeout=120):
    port = free_port()
    procs = []
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port),
                   LOCAL_RANK="0")
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "dist_agg_worker.py"), mode], env=env,
                                      stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    outs = []
    for p in procs:
        try:
            out, _ = p.communicate(timeout=timeout)
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
        outs.append((p.returncode, out.decode(errors="replace")))
    for rc, out in outs:
        assert rc == 0, out[-3000:]


# ---- CPU -------------------------------------------------------------------------------------------

def test_prototype_is_declared_and_bound():
    src = open(os.path.join(ROOT, "include", "qeh.h")).read()
    assert "#define QEH_ABI_VERSION 1" in src  # additive change
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"^\s*int\s+qeh_avg_finalize\s*\(([^)]*)\)\s*;", code, flags=re.M)
    assert m, "qeh_avg_finalize is not declared in include/qeh.h"
    assert m.group(1).count("qeh_column") == 3 and "qeh_ctx" in m.group(1)
    assert "qeh_avg_finalize" in abi.SIGNATURES
    restype, argtypes = abi.SIGNATURES["qeh_avg_finalize"]
    assert len(argtypes) == 5
    lib = qe_hip.load()
    assert hasattr(lib, "qeh_avg_finalize")
    assert hasattr(qe_hip.Context, "avg_finalize")
    assert lib.qeh_abi_version() == 1


def host_recipe(shards, aggs, groups):
    """Host model of the distributed plan for `aggs` over per-rank (key, columns): per-rank partials
    (SUM of an Int32 column wrapped to 32 bits and widened, as the device's and the reference's is),
    merged by FINAL_OF, AVG finished as qeh_avg_finalize does -- the Int32 wrap applied once, at the
    end.  Returns one {group: value-or-None} per requested aggregate."""
    from qe_hip.distributed import FINAL_OF, expand_avg
    partial, recipe = expand_avg(aggs, max_partials=None)
    merge = {AF.Sum: lambda a, b: a + b, AF.Min: min, AF.Max: max}
    state = [dict() for _ in partial]
    for key, cols in shards:
        for g in np.unique(key):
            for j, (f, c) in enumerate(partial):
                v = cols[c][key == g]
                if f == AF.Count:
                    p = int(len(v))
                elif f == AF.Sum:
                    p = int(v.sum(dtype=np.int64).astype(np.int32)) if v.dtype == np.int32 else \
                        (float(v.sum()) if v.dtype.kind == "f" else int(v.sum()))
                else:
                    p = {AF.Min: v.min, AF.Max: v.max}[f]().item()
                state[j][g] = merge[FINAL_OF[f]](state[j][g], p) if g in state[j] else p
    out = []
    for r in recipe:
        if isinstance(r, int):
            out.append(state[r])
            continue
        si, ci, c = r
        dt = shards[0][1][c].dtype
        res = {}
        for g in range(groups):
            s, n = state[si].get(g), state[ci].get(g, 0)
            if dt == np.int32 and s is not None:
                s = int(np.int64(s).astype(np.int32))
            res[g] = None if n <= 0 else float(np.float64(s) / np.float64(n))
        out.append(res)
    return out


def test_expand_avg_table():
    from qe_hip.distributed import MAX_AGGS_PER_OPERATOR, expand_avg
    assert MAX_AGGS_PER_OPERATOR == 8
    assert expand_avg([(AF.Avg, 2)]) == ([(AF.Sum, 2), (AF.Count, 2)], [(0, 1, 2)])
    # what the caller asked for is reused, not copied
    assert expand_avg([(AF.Sum, 2), (AF.Avg, 2), (AF.Count, 2)]) == ([(AF.Sum, 2), (AF.Count, 2)], [0, (0, 1, 2), 1])
    assert expand_avg([(AF.Count, 2), (AF.Avg, 2)]) == ([(AF.Count, 2), (AF.Sum, 2)], [0, (1, 0, 2)])
    assert expand_avg([(AF.Avg, 0), (AF.Avg, 1), (AF.Min, 0)]) == (
        [(AF.Sum, 0), (AF.Count, 0), (AF.Sum, 1), (AF.Count, 1), (AF.Min, 0)], [(0, 1, 0), (2, 3, 1), 4])
    assert expand_avg([(AF.Avg, 1), (AF.Avg, 1)]) == ([(AF.Sum, 1), (AF.Count, 1)], [(0, 1, 1), (0, 1, 1)])
    # no AVG: the list itself, identity recipe (repeats and order kept)
    plain = [(AF.Sum, 2), (AF.Count, 2), (AF.Max, 2), (AF.Sum, 2)]
    assert expand_avg(plain) == (plain, [0, 1, 2, 3])
    assert expand_avg([]) == ([], [])
    # eight partials fit one device operator, nine do not
    four = [(AF.Avg, c) for c in range(4)]
    assert len(expand_avg(four)[0]) == 8
    for too_many in (four + [(AF.Min, 0)], [(AF.Sum, c) for c in range(9)]):
        with pytest.raises(abi.QehError) as e:
            expand_avg(too_many)
        assert e.value.status == abi.QEH_E_UNSUPPORTED and "8" in e.value.message
    # qeh_hash_aggregate runs longer lists in chunks: group_by and aggregate lift the bound
    assert len(expand_avg(four + [(AF.Min, 0)], max_partials=None)[0]) == 9


def test_recipe_host_model_equals_numpy_over_the_whole():
    r = np.random.default_rng(21)
    n, groups = 10_000, 13
    shards = []
    for q in range(3):
        key = r.integers(0, groups - 1, n)
        i64 = r.integers(-10 ** 12, 10 ** 12, n).astype(np.int64)
        i32 = r.integers(-1000, 1000, n).astype(np.int32)
        f64 = r.integers(-(2 ** 20) + 1, 2 ** 20, n).astype(np.float64) / 1024.0
        key[:5] = groups - 1  # five 2**30 per shard: 15 * 2**30 crosses 2**31 (and 2**32)
        i32[:5] = 2 ** 30
        shards.append((key, [i64, i32, f64]))
    aggs = [(AF.Avg, 0), (AF.Sum, 0), (AF.Avg, 1), (AF.Avg, 2), (AF.Count, 2), (AF.Min, 1)]
    got = host_recipe(shards, aggs, groups)
    K = np.concatenate([k for k, _ in shards])
    C = [np.concatenate([c[j] for _, c in shards]) for j in range(3)]
    for g in range(groups):
        sel = K == g
        cnt = int(sel.sum())
        assert cnt > 0
        assert got[0][g] == float(np.float64(C[0][sel].sum()) / np.float64(cnt))
        assert got[1][g] == int(C[0][sel].sum())
        wrapped = C[1][sel].sum(dtype=np.int64).astype(np.int32)  # the reference's i32 compute::sum
        assert got[2][g] == float(np.float64(wrapped) / np.float64(cnt))
        assert got[3][g] == float(C[2][sel].sum() / np.float64(cnt))  # exactly summable: any order
        assert got[4][g] == cnt
        assert got[5][g] == int(C[1][sel].min())
    total = C[1][K == groups - 1].sum(dtype=np.int64)
    assert total == 15 * 2 ** 30 and got[2][groups - 1] == float(-(2 ** 30)) / 15


# ---- qeh_avg_finalize alone --------------------------------------------------------------------------

LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 100_003]


def finalize_inputs(n, kind, seed):
    """(sum values, count values, count validity) of one case: counts in 1..9 with 0 at rows 0, 63, 64
    and the last, one NULL count; float sums carry +-0.0, +-inf and NaN, Int32-input sums the values
    whose 32-bit wrap changes them."""
    r = np.random.default_rng(seed)
    cnt = r.integers(1, 10, n).astype(np.int64)
    for z in (0, 63, 64, n - 1):
        if 0 <= z < n:
            cnt[z] = 0
    cm = np.ones(n, bool)
    if n > 2:
        cm[n // 2] = False
    if kind == "f64":
        s = r.standard_normal(n) * 1e3
        for i, x in enumerate([0.0, -0.0, np.inf, -np.inf, np.nan]):
            if n > 1 + i:
                s[(1 + i) % n] = x  # rows 1..5: valid counts (row 0's is 0)
            if n > 70 + i:
                s[66 + i] = x
    else:
        s = r.integers(-2 ** 40, 2 ** 40, n).astype(np.int64)
        if kind == "i32":
            s = r.integers(-2 ** 33, 2 ** 33, n).astype(np.int64)
            for i, x in enumerate([2 ** 31, 2 ** 32 + 5, -2 ** 31 - 1]):
                if n > 1 + i:
                    s[1 + i] = x
                if n > 70 + i:
                    s[66 + i] = x
    return s, cnt, cm


def finalize_expected(s, sm, cnt, cm, kind):
    v = s.astype(np.int32).astype(np.float64) if kind == "i32" else s.astype(np.float64)
    if sm is not None:
        v = np.where(sm, v, 0.0)  # a NULL sum reads as 0 (operators.rs:772 unwrap_or(0))
    valid = cnt > 0 if cm is None else (cnt > 0) & cm
    with np.errstate(all="ignore"):
        return v / cnt.astype(np.float64), valid


def check_finalize(ctx, n, kind, sum_bitmap, count_bitmap, sliced, seed):
    s, cnt, cm = finalize_inputs(n, kind, seed)
    if not count_bitmap:
        cm = None
    sm = (np.random.default_rng(seed + 1).random(n) > 0.25) if sum_bitmap else None
    pad = 3 if sliced else 0
    def up(v, m):
        if not pad:
            return ctx.upload(v, m)
        whole = ctx.upload(np.concatenate([np.full(pad, 77, v.dtype), v, np.full(2, 78, v.dtype)]),
                           None if m is None else np.concatenate([np.ones(pad, bool), m, np.zeros(2, bool)]))
        return ctx.slice(whole, pad, len(v))
    dt = {"i64": abi.DT_INT64, "i32": abi.DT_INT32, "f64": abi.DT_FLOAT64}[kind]
    out = ctx.avg_finalize(up(s, sm), up(cnt, cm), dt)
    want, valid = finalize_expected(s, sm, cnt, cm, kind)
    what = (n, kind, sum_bitmap, count_bitmap, sliced)
    assert out.dtype == abi.DT_FLOAT64 and len(out) == n and out.c.offset == 0, what
    assert out.c.null_count == n - int(valid.sum()), (what, out.c.null_count)
    gv, gm = out.to_numpy()
    assert gm is not None and np.array_equal(gm, valid), what
    assert np.array_equal(gv.view(np.int64)[valid], want.view(np.int64)[valid]), what


@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_avg_finalize_vs_numpy(ctx, n):
    seed = 1000 + n
    for kind in ("i64", "f64", "i32"):
        for sum_bitmap in (False, True):
            check_finalize(ctx, n, kind, sum_bitmap, True, False, seed)
        check_finalize(ctx, n, kind, False, False, False, seed)
        check_finalize(ctx, n, kind, True, True, True, seed)  # both inputs sliced at offset 3
    # Float32 inputs take the Float64 path (their SUM is Float64)
    s, cnt, cm = finalize_inputs(n, "f64", seed)
    out = ctx.avg_finalize(ctx.upload(s), ctx.upload(cnt, cm), abi.DT_FLOAT32)
    want, valid = finalize_expected(s, None, cnt, cm, "f64")
    gv, gm = out.to_numpy()
    assert np.array_equal(gm, valid) and np.array_equal(gv.view(np.int64)[valid], want.view(np.int64)[valid])


@pytest.mark.gpu
def test_avg_finalize_is_one_kernel_and_refuses_other_types(ctx):
    s, cnt, cm = finalize_inputs(1000, "i64", 5)
    ctx.timing(True)
    ctx.timing_reset()
    ctx.avg_finalize(ctx.upload(s), ctx.upload(cnt, cm), abi.DT_INT64)
    launches = ctx.kernel_time("avg_finalize")[1]
    ctx.timing(False)
    assert launches == 1
    i64, f64, i32 = ctx.upload(s), ctx.upload(s.astype(np.float64)), ctx.upload(s.astype(np.int32))
    c = ctx.upload(cnt)
    for args in ((i32, c, abi.DT_INT32), (i64, f64, abi.DT_INT64), (i64, ctx.upload(cnt.astype(np.int32)), abi.DT_INT64),
                 (i64, c, abi.DT_UTF8), (i64, c, abi.DT_BOOL), (i64, c, abi.DT_DATE32), (i64, c, abi.DT_TIMESTAMP_US),
                 (f64, c, abi.DT_INT32), (f64, c, abi.DT_INT64), (i64, c, abi.DT_FLOAT64)):
        with pytest.raises(abi.QehError) as e:
            ctx.avg_finalize(*args)
        assert e.value.status == abi.QEH_E_TYPE, args[2]
    with pytest.raises(abi.QehError) as e:
        ctx.avg_finalize(i64, ctx.upload(cnt[:-1]), abi.DT_INT64)
    assert e.value.status == abi.QEH_E_INVALID
    assert ctx.lib.qeh_avg_finalize(ctx.h, None, None, abi.DT_INT64, None) == abi.QEH_E_INVALID


# ---- the distributed plans (ranks as processes on one GPU) -------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 2, 3])
def test_group_by_with_avg(world):
    """5 000 + 17 * rank rows per rank, 97 Int64 groups, AVG of Int64, nullable Float64, Int32 and
    Float32 inputs beside SUM / COUNT / MIN; a group whose Float64 values are NULL everywhere, one on
    one rank only, one NULL on rank 0 only, one whose Int32 sum overflows; then two groups, so that a
    rank owns none.  Equal to the oracle over the concatenation, bit for bit."""
    launch("group_by", world)


@pytest.mark.gpu
def test_joins_with_avg_keep_their_final_stage():
    """Shuffle and sharded broadcast joins (120 000 fact rows per rank, 30 000 dimension rows, 97
    groups) with [AVG, COUNT] (dense final) and [AVG, AVG, float MAX] (shuffled final), exact."""
    launch("joins", 2)


@pytest.mark.gpu
def test_items_forms_keep_avg():
    """[AVG(v)] over a unique dimension of 3 145 728 keys: the broadcast and the shuffle join both
    stay on their items form (a float-SUM lane and a COUNT lane), exact."""
    launch("items", 2)


@pytest.mark.gpu
@pytest.mark.parametrize("world", [1, 2])
def test_aggregate_without_group_by(world):
    """DistributedExecutor.aggregate: [AVG, SUM, COUNT, MIN, MAX] of each of the four input types;
    input_batches = 0; a column NULL everywhere; rank 1 with zero rows.  Rank 0's row equals the
    oracle's, the other ranks return zero-row columns of the same types."""
    launch("aggregate", world)
