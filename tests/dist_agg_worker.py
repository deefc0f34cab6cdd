"""One rank of the multi-process tests of distributed AVG and of DistributedExecutor.aggregate
(launched by tests/test_distributed_avg.py as separate processes; RANK / WORLD_SIZE / MASTER_* in
the environment).  Every rank computes on cuda:0, collectives over gloo.

Every float input is exactly summable in any order, so every comparison with the oracle is exact:
  * Float64 values are k / 1024 with integer |k| < 2**20: fewer than 2**19 rows job-wide (the largest
    job here has 400 000) keep every sum below 2**39 units of 1/1024, far inside 53 bits;
  * Float32 values are multiples of 0.25 in [-64, 64], at most 2**8 units each: fewer than 2**14 rows
    job-wide (the largest Float32 job here has 15 051) keep every sum below 2**22 units, inside
    float32's 24 bits, so the oracle's float32 accumulation, the device's partials and their float64
    merge agree to the bit."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "query-engine_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

GROUPS = 97
G_ALL_NULL, G_ONE_RANK, G_NULL_ON_0, G_OVERFLOW = 90, 91, 92, 93


def f64_exact(r, n):
    return r.integers(-(2 ** 20) + 1, 2 ** 20, n).astype(np.float64) / 1024.0


def shard(rank, overflow=True):
    """This rank's rows: the Int64 group key, then (values, validity-or-None) of the four inputs --
    Int64, nullable Float64 (20 % NULL), Int32, Float32.  Group 90's Float64 values are NULL on every
    rank, group 91 exists on rank 0 only, group 92's Float64 values are NULL on rank 0 and valid
    elsewhere, and (with `overflow`) group 93 is five rows of Int32 2**30 per rank."""
    r = np.random.default_rng(700 + rank)
    n = 5000 + 17 * rank
    key = r.integers(0, GROUPS, n).astype(np.int64)
    a = r.integers(-1000, 1000, n).astype(np.int64)
    b = f64_exact(r, n)
    bm = r.random(n) > 0.2
    c = r.integers(-1000, 1000, n).astype(np.int32)
    d = (r.integers(-256, 257, n) * 0.25).astype(np.float32)
    if rank != 0:
        key[key == G_ONE_RANK] = 5
    key[key == G_OVERFLOW] = 7
    if overflow:
        key[:5] = G_OVERFLOW
        c[:5] = 2 ** 30
    bm[key == G_ALL_NULL] = False
    bm[key == G_NULL_ON_0] = rank != 0
    return key, [(a, None), (b, bm), (c, None), (d, None)]


def whole(world, overflow=True, keep=None):
    """The concatenation of every rank's shard (ranks not in `keep` contribute no rows)."""
    parts = [shard(q, overflow) for q in range(world) if keep is None or q in keep]
    key = np.concatenate([p[0] for p in parts])
    cols = []
    for j in range(4):
        v = np.concatenate([p[1][j][0] for p in parts])
        m = None if parts[0][1][j][1] is None else np.concatenate([p[1][j][1] for p in parts])
        cols.append((v, m))
    return key, cols


def bits(v):
    v = np.ascontiguousarray(v)
    return v.view({4: np.int32, 8: np.int64}[v.dtype.itemsize]) if v.dtype.kind == "f" else v


def assert_column_exact(got, want, what):
    """(values, validity) pairs: same dtype and length, same NULLs, same value bits at valid rows."""
    (gv, gm), (wv, wm) = got, want
    gm = np.ones(len(gv), bool) if gm is None else np.asarray(gm, bool)
    wm = np.ones(len(wv), bool) if wm is None else np.asarray(wm, bool)
    assert gv.dtype == wv.dtype, (what, gv.dtype, wv.dtype)
    assert len(gv) == len(wv), (what, len(gv), len(wv))
    assert np.array_equal(gm, wm), (what, "NULL masks differ", np.nonzero(gm != wm)[0][:8])
    bad = np.nonzero(bits(gv)[gm] != bits(wv)[wm])[0]
    assert len(bad) == 0, (what, gv[gm][bad[:4]], wv[wm][bad[:4]])


def assert_grouped_exact(res, wk, wa, what):
    """res: gathered [(key, mask), (agg, mask)...] in any row order; wk / wa: the oracle's."""
    go = np.argsort(res[0][0], kind="stable")
    wo = np.argsort(wk[0][0], kind="stable")
    assert np.array_equal(res[0][0][go], wk[0][0][wo]), (what, "group keys differ")
    assert len(res) - 1 == len(wa)
    for j, (w, g) in enumerate(zip(wa, res[1:])):
        assert_column_exact((g[0][go], g[1][go]), (w[0][wo], w[1][wo]), f"{what}: aggregate {j}")


def device_executor():
    """The RCCL path's device-tensor code over gloo: the library on a torch stream, CUDA payloads."""
    import qe_hip
    from qe_hip.distributed import DistributedExecutor
    torch.cuda.set_device(0)
    s = torch.cuda.Stream()
    torch.cuda.set_stream(s)
    ctx = qe_hip.Context(0)
    ctx.set_stream(s.cuda_stream)
    return ctx, DistributedExecutor(ctx, device="cuda")


def close(ctx):
    torch.cuda.synchronize()
    ctx.set_stream(0)
    ctx.close()


def mode_group_by(rank, world):
    """group_by with AVG over the four input types, against the oracle over the concatenation.  World 2
    runs with device payloads, worlds 1 and 3 with host payloads (both rehearsals of the RCCL path)."""
    import qe_hip
    import oracle_bind as ob
    from qe_hip import AggregateFunction as AF
    from qe_hip.distributed import DistributedExecutor
    if world == 2:
        ctx, dx = device_executor()
    else:
        ctx = qe_hip.Context(0)
        dx = DistributedExecutor(ctx)
    aggs = [(AF.Avg, 0), (AF.Sum, 0), (AF.Avg, 1), (AF.Count, 1), (AF.Avg, 2), (AF.Avg, 3), (AF.Min, 0)]
    key, cols = shard(rank)
    keys, out, g = dx.group_by([ctx.upload(key)], [ctx.upload(v, m) for v, m in cols], aggs)
    assert len(out) == len(aggs) and all(len(c) == g for c in keys + out)
    assert [c.dtype for c in out] == [qe_hip.abi.DT_FLOAT64, qe_hip.abi.DT_INT64, qe_hip.abi.DT_FLOAT64,
                                      qe_hip.abi.DT_INT64, qe_hip.abi.DT_FLOAT64, qe_hip.abi.DT_FLOAT64,
                                      qe_hip.abi.DT_INT64]
    res = dx.gather_to_root(keys + out)
    if rank == 0:
        K, C = whole(world)
        wk, wa, wg, _ = ob.hash_aggregate([ob.HostCol(K)], [ob.HostCol(v, m) for v, m in C], aggs)
        assert wg == GROUPS
        assert_grouped_exact(res, wk, wa, f"group_by world {world}")
        # the special groups are what they claim to be
        o = np.argsort(wk[0][0])
        avg_b, avg_c = (wa[2][0][o], wa[2][1][o]), (wa[4][0][o], wa[4][1][o])
        assert not avg_b[1][G_ALL_NULL] and avg_b[1][G_NULL_ON_0] == (world > 1)
        total = np.int64(5 * world * 2 ** 30)
        assert avg_c[0][G_OVERFLOW] == float(total.astype(np.int32)) / (5 * world) and total > 2 ** 31
    # a rank that owns no group still returns typed columns: 2 groups over up to 3 ranks
    few = (key % 2).astype(np.int64)
    keys, out, g = dx.group_by([ctx.upload(few)], [ctx.upload(v, m) for v, m in cols], [(AF.Avg, 3), (AF.Max, 2)])
    assert [c.dtype for c in out] == [qe_hip.abi.DT_FLOAT64, qe_hip.abi.DT_INT32] and all(len(c) == g for c in out)
    res = dx.gather_to_root(keys + out)
    if rank == 0:
        K, C = whole(world)
        wk, wa, wg, _ = ob.hash_aggregate([ob.HostCol((K % 2).astype(np.int64))], [ob.HostCol(v, m) for v, m in C],
                                          [(AF.Avg, 3), (AF.Max, 2)])
        assert_grouped_exact(res, wk, wa, f"two groups, world {world}")
    if world == 2:
        close(ctx)
    else:
        ctx.close()


def join_shards(rank, world, n=120_000, nd=30_000, groups=GROUPS):
    """dist_worker.metric_shards' shapes (fact keys with NULLs and misses, a dimension split by rows
    with one repeated key) with v drawn from the exactly summable Float64 set."""
    def fact(q):
        g = np.random.default_rng(300 + q)
        x = g.integers(0, 100, n).astype(np.int64)
        k = g.integers(0, nd + 1000, n).astype(np.int64)
        km = g.random(n) > 0.02
        return x, k, km, f64_exact(g, n)
    dk_all = np.random.default_rng(5).permutation(nd).astype(np.int64)
    dk_all[11] = dk_all[12]
    dg_all = np.random.default_rng(6).integers(0, groups, nd).astype(np.int64)
    b = np.linspace(0, nd, world + 1).astype(int)
    everything = [np.concatenate(c) for c in zip(*[fact(q) for q in range(world)])]
    return fact(rank), (dk_all[b[rank]:b[rank + 1]], dg_all[b[rank]:b[rank + 1]]), everything, (dk_all, dg_all)


def mode_joins(rank, world):
    """The shuffle join and the sharded broadcast join with AVG; the final stage each list takes is
    the one its SUM + COUNT expansion takes."""
    import oracle_bind as ob
    from qe_hip import AggregateFunction as AF, BinaryOp, binop, col, lit
    ctx, dx = device_executor()
    (x, k, km, v), (dk, dg), (X, K, KM, V), (DK, DG) = join_shards(rank, world)
    pred = binop(col(0), BinaryOp.Greater, lit(49))
    fact = [ctx.upload(x), ctx.upload(k, km), ctx.upload(v)]
    for aggs, final in (([(AF.Avg, 2), (AF.Count, 2)], "dense"), ([(AF.Avg, 2), (AF.Avg, 0), (AF.Max, 2)], "shuffle")):
        want = ob.join_filter_aggregate([ob.HostCol(X), ob.HostCol(K, KM), ob.HostCol(V)], 1, pred, ob.HostCol(DK),
                                        [ob.HostCol(DG)], aggs) if rank == 0 else None
        for name, fn in (("shuffle", dx.join_filter_aggregate_shuffle),
                         ("broadcast", lambda *a: dx.join_filter_aggregate_broadcast(*a, build_sharded=True))):
            keys, out, g = fn(fact, 1, pred, ctx.upload(dk), [ctx.upload(dg)], aggs)
            if name == "broadcast":
                assert dx.last_final == final, (dx.last_final, final)
            assert len(out) == len(aggs)
            res = dx.gather_to_root(keys + out)
            if rank == 0:
                assert_grouped_exact(res, want[0], want[1], f"{name} join {aggs}")
    close(ctx)


def mode_items(rank, world):
    """The smallest shape the items forms accept (a unique, non-null Int64 dimension over
    ITEMS_MIN_TABLE_BYTES / 2 keys, sharded by rows) with AVG: both joins stay on the items form."""
    import oracle_bind as ob
    from qe_hip import AggregateFunction as AF, BinaryOp, binop, col, lit
    from qe_hip.distributed import DistributedExecutor
    R, groups, n = DistributedExecutor.ITEMS_MIN_TABLE_BYTES // 2, 64, 200_000
    assert R == 3_145_728
    dk_all = np.random.default_rng(11).permutation(R).astype(np.int64)
    dg_all = np.random.default_rng(12).integers(0, groups, R).astype(np.int64)
    b = np.linspace(0, R, world + 1).astype(int)

    def fact(q):
        g = np.random.default_rng(400 + q)
        return g.integers(0, 100, n).astype(np.int64), g.integers(0, R, n).astype(np.int64), f64_exact(g, n)
    ctx, dx = device_executor()
    x, k, v = fact(rank)
    pred = binop(col(0), BinaryOp.Greater, lit(49))
    aggs = [(AF.Avg, 2)]
    cols = [ctx.upload(x), ctx.upload(k), ctx.upload(v)]
    dkc, dgc = ctx.upload(dk_all[b[rank]:b[rank + 1]]), ctx.upload(dg_all[b[rank]:b[rank + 1]])
    if rank == 0:
        X, K, V = (np.concatenate(c) for c in zip(*[fact(q) for q in range(world)]))
        want = ob.join_filter_aggregate([ob.HostCol(X), ob.HostCol(K), ob.HostCol(V)], 1, pred, ob.HostCol(dk_all),
                                        [ob.HostCol(dg_all)], aggs)
    keys, out, g = dx.join_filter_aggregate_broadcast(cols, 1, pred, dkc, [dgc], aggs, build_sharded=True)
    assert dx.last_build == "items", dx.last_build
    res = dx.gather_to_root(keys + out)
    if rank == 0:
        assert_grouped_exact(res, want[0], want[1], "broadcast items form")
    keys, out, g = dx.join_filter_aggregate_shuffle(cols, 1, pred, dkc, [dgc], aggs)
    assert dx.last_shuffle == "items", dx.last_shuffle
    res = dx.gather_to_root(keys + out)
    if rank == 0:
        assert_grouped_exact(res, want[0], want[1], "shuffle items form")
    close(ctx)


def mode_aggregate(rank, world):
    """DistributedExecutor.aggregate (no GROUP BY): rank 0's row against the oracle over the
    concatenation, zero-row columns of the same types elsewhere.  The rows are test 4's without
    group 93's 2**30s: the job-wide SUM(Int32) would overflow, and the distributed final stage does
    not wrap SUM(Int32) to 32 bits -- AVG's wrap is checked in mode_group_by."""
    import qe_hip
    import oracle_bind as ob
    from qe_hip import AggregateFunction as AF
    from qe_hip.distributed import DistributedExecutor
    ctx = qe_hip.Context(0)
    dx = DistributedExecutor(ctx)

    def check(cols, WC, what, input_batches=1):
        for c in range(4):
            aggs = [(AF.Avg, c), (AF.Sum, c), (AF.Count, c), (AF.Min, c), (AF.Max, c)]
            out, g = dx.aggregate([ctx.upload(v, m) for v, m in cols], aggs, input_batches)
            _, wa, wg, wdts = ob.hash_aggregate([], [ob.HostCol(v, m) for v, m in WC], aggs, input_batches)
            shapes = [None] * world
            dist.all_gather_object(shapes, [(col.dtype, len(col)) for col in out])
            assert len(out) == len(aggs)
            assert [d for d, _ in shapes[rank]] == [d for d, _ in shapes[0]], (what, shapes)
            assert all(n == (wg if q == 0 else 0) for q in range(world) for _, n in shapes[q]), (what, shapes, wg)
            assert g == (wg if rank == 0 else 0)
            if rank == 0 and wg:
                assert [col.dtype for col in out] == list(wdts)
                for j, col in enumerate(out):
                    assert_column_exact(col.to_numpy(), wa[j], f"{what}: column {c}, aggregate {j}")
        return wa

    _, cols = shard(rank, overflow=False)
    _, WC = whole(world, overflow=False)
    check(cols, WC, f"aggregate world {world}")
    # no batch anywhere: no row anywhere (executor.rs:178)
    check(cols, WC, "input_batches=0", input_batches=0)
    # the Float64 column NULL everywhere: AVG, SUM, MIN and MAX are NULL, COUNT is 0
    null_b = [cols[0], (cols[1][0], np.zeros(len(cols[1][0]), bool))] + cols[2:]
    WN = [WC[0], (WC[1][0], np.zeros(len(WC[1][0]), bool))] + WC[2:]
    check(null_b, WN, "a column NULL everywhere")
    out, g = dx.aggregate([ctx.upload(v, m) for v, m in null_b], [(AF.Avg, 1), (AF.Count, 1)])
    if rank == 0:
        (av, am), (cv, cm) = out[0].to_numpy(), out[1].to_numpy()
        assert g == 1 and not am[0] and cv[0] == 0 and (cm is None or cm[0])
    if world > 1:
        # rank 1 holds zero rows (and no bitmap, where rank 0's Float64 column has one)
        empty = [(v[:0], None) for v, _ in cols]
        _, WE = whole(world, overflow=False, keep=[q for q in range(world) if q != 1])
        check(empty if rank == 1 else cols, WE, "rank 1 empty")
    ctx.close()


def main():
    mode = sys.argv[1]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        {"group_by": mode_group_by, "joins": mode_joins, "items": mode_items, "aggregate": mode_aggregate}[mode](rank, world)
        dist.barrier()
    finally:
        dist.destroy_process_group()
    print(f"rank {rank} ok")


if __name__ == "__main__":
    main()
