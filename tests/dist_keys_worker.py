"""One rank of the multi-process tests of Utf8 and temporal keys in the distributed GROUP BY, window,
sort and join (launched by tests/test_distributed_keys.py as separate processes; RANK / WORLD_SIZE /
MASTER_* in the environment).  Every rank computes on cuda:0, collectives over gloo.

Every case compares with the same operator run on one device over the rank-major concatenation of
all shards, which every rank rebuilds from the seeds.  Worlds 1 and 3 run DistributedExecutor(ctx),
the host-staged path; world 2 runs every case on that and on DistributedExecutor(ctx, device="cuda").
The host-staged Utf8 path decodes strings, so the data is valid UTF-8; "é", "ß", "日本" and Cyrillic
words bring bytes >= 0x80.  Float64 aggregate inputs are k / 1024 with integer |k| < 2**20 (exactly
summable in any order, as in tests/dist_agg_worker.py), so every comparison is exact."""
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "query-engine_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

ONLY0 = "only-on-rank-zero"
SPECIAL = ["", "é", "ß", "日本", "日本語", "straße", "abcdefgh-1", "abcdefgh-2", "a", "ab", "abc", ONLY0]
VOCAB = np.array(SPECIAL + [("клю%d" % i) if i % 5 == 0 else "w%03d" % i for i in range(97 - len(SPECIAL))], dtype=object)
assert len(set(VOCAB)) == 97


def f64_exact(r, n):
    return r.integers(-(2 ** 20) + 1, 2 ** 20, n).astype(np.float64) / 1024.0


def shard(rank):
    """This rank's rows as {name: (values, validity-or-None)}: s Utf8 (5 % NULL, 97 strings, one on rank
    0 only), s10 the same strings with 10 % NULL, k2 Int64 in 0..4, a Int64, b Float64 (20 % NULL), and
    the temporal columns d32 (Date32), tus / tns / tms (Timestamp us / ns / ms) and d64 (Date64) as
    their physical integers, negative values and 5 % NULL included."""
    r = np.random.default_rng(900 + rank)
    n = 5000 + 17 * rank
    s = VOCAB[r.integers(0, len(VOCAB), n)]
    if rank != 0:
        s[s == ONLY0] = "w001"
    else:
        s[:3] = ONLY0
    return {
        "s": (s, r.random(n) > 0.05), "s10": (s, r.random(n) > 0.10),
        "k2": (r.integers(0, 5, n).astype(np.int64), None),
        "a": (r.integers(-1000, 1000, n).astype(np.int64), None),
        "b": (f64_exact(r, n), r.random(n) > 0.2),
        "d32": (r.integers(-20, 20, n).astype(np.int32), r.random(n) > 0.05),
        "tus": (r.integers(-50, 50, n).astype(np.int64) * 1_000_003, r.random(n) > 0.05),
        "tns": (r.integers(-10 ** 12, 10 ** 12, n).astype(np.int64), None),
        "tms": (r.integers(-10 ** 9, 10 ** 9, n).astype(np.int64), r.random(n) > 0.05),
        "d64": (r.integers(-300, 300, n).astype(np.int64) * 86_400_000, r.random(n) > 0.05),
    }


def cut(table, rows):
    return {k: (v[rows], None if m is None else m[rows]) for k, (v, m) in table.items()}


def concat(tables):
    out = {}
    for k in tables[0]:
        v = np.concatenate([t[k][0] for t in tables])
        if tables[0][k][0].dtype == object:
            v = v.astype(object)
        out[k] = (v, None if tables[0][k][1] is None else np.concatenate([t[k][1] for t in tables]))
    return out


def job(rank, world, empty_rank=None, edit=None):
    """(this rank's table, the whole job's table, this rank's first global row); `edit` rewrites every
    shard, `empty_rank` holds zero rows."""
    shards = [shard(q) for q in range(world)]
    if edit is not None:
        shards = [edit(t) for t in shards]
    shards = [cut(t, slice(0, 0)) if q == empty_rank else t for q, t in enumerate(shards)]
    first = sum(len(t["a"][0]) for t in shards[:rank])
    return shards[rank], concat(shards), first


def make_uploader(ctx):
    from qe_hip import abi
    temporal = {"d32": abi.DT_DATE32, "tus": abi.DT_TIMESTAMP_US, "tns": abi.DT_TIMESTAMP_NS, "tms": abi.DT_TIMESTAMP_MS,
                "d64": abi.DT_DATE64}

    def up(table, name):
        v, m = table[name]
        return ctx.upload(v, m, dtype=temporal[name]) if name in temporal else ctx.upload(v, m)
    up.dtypes = temporal
    return up


def canon(col):
    """One column's (values, validity) as a list of Python values that compare exactly: str, int, the
    bits of a float, the integer of a datetime64; None for NULL."""
    v, m = col
    v = np.asarray(v)
    if v.dtype.kind in "Mf":
        v = v.view(np.int64)
    items = v.tolist()
    if m is not None:
        items = [x if ok else None for x, ok in zip(items, m)]
    return items


def rows_of(cols):
    return list(zip(*[canon(c) for c in cols])) if cols else []


def row_key(t):
    return tuple((x is None, 0 if x is None else x) for x in t)


def assert_col_equal(got, want, what):
    assert np.asarray(got[0]).dtype == np.asarray(want[0]).dtype, (what, got[0].dtype, want[0].dtype)
    g, w = canon(got), canon(want)
    assert len(g) == len(w), (what, len(g), len(w))
    bad = [i for i in range(len(g)) if g[i] != w[i]]
    assert not bad, (what, len(bad), [(i, g[i], w[i]) for i in bad[:4]])


def setup(world):
    """(ctx, [(name, executor)]): at world 2 the library runs on a torch stream and both the host-staged
    and the device-payload executor are exercised; else the host-staged one."""
    import qe_hip
    from qe_hip.distributed import DistributedExecutor
    if world == 2:
        torch.cuda.set_device(0)
        s = torch.cuda.Stream()
        torch.cuda.set_stream(s)
        ctx = qe_hip.Context(0)
        ctx.set_stream(s.cuda_stream)
        return ctx, [("host", DistributedExecutor(ctx)), ("cuda", DistributedExecutor(ctx, device="cuda"))]
    ctx = qe_hip.Context(0)
    return ctx, [("host", DistributedExecutor(ctx))]


def close(ctx, world):
    if world == 2:
        torch.cuda.synchronize()
        ctx.set_stream(0)
    ctx.close()


def check_group_by(ctx, dx, up, mine, everything, key_names, aggs, agg_inputs, what, min_groups=1):
    """The ranks' groups are disjoint and their union equals the single-device aggregate, row for row."""
    keys, out, g = dx.group_by([up(mine, k) for k in key_names], [up(mine, c) for c in agg_inputs], aggs)
    wk, wa, wg = ctx.hash_aggregate([up(everything, k) for k in key_names], [up(everything, c) for c in agg_inputs], aggs)
    assert len(keys) == len(key_names) and len(out) == len(aggs) and all(len(c) == g for c in keys + out), what
    assert [c.dtype for c in keys] == [c.dtype for c in wk], (what, [c.dtype for c in keys])
    assert [c.dtype for c in out] == [c.dtype for c in wa], (what, [c.dtype for c in out])
    local = rows_of([c.to_numpy() for c in keys + out])
    parts = [None] * dx.world
    dist.all_gather_object(parts, local)
    nk = len(key_names)
    seen = {}
    for q, part in enumerate(parts):
        for t in part:
            assert seen.setdefault(t[:nk], q) == q, (what, "a group on two ranks", t[:nk])
    union = sorted((t for part in parts for t in part), key=row_key)
    want = sorted(rows_of([c.to_numpy() for c in wk + wa]), key=row_key)
    assert wg >= min_groups and len(want) == wg
    assert union == want, (what, len(union), len(want), [(a, b) for a, b in zip(union, want) if a != b][:3])
    return parts


def mode_group_by(rank, world):
    from qe_hip import AggregateFunction as AF
    ctx, executors = setup(world)
    up = make_uploader(ctx)
    aggs = [(AF.Sum, 0), (AF.Count, 0), (AF.Min, 0), (AF.Avg, 1)]
    for name, dx in executors:
        mine, everything, _ = job(rank, world)
        for key_names in (["s"], ["s", "k2"], ["k2", "s"]):
            parts = check_group_by(ctx, dx, up, mine, everything, key_names, aggs, ["a", "b"],
                                   f"{name} group_by {key_names} world {world}", min_groups=98)
            if key_names == ["s"]:
                flat = [t[0] for part in parts for t in part]
                assert len(flat) == 98 and None in flat and ONLY0 in flat and "" in flat and "日本" in flat  # 97 + the NULL group
        # two groups job-wide: at world 3 a rank owns none and still exchanges typed columns

        def two(t):
            t = dict(t)
            t["s"] = (np.where(t["k2"][0] % 2 == 0, "abcdefgh-1", "abcdefgh-2").astype(object), None)
            return t
        mine, everything, _ = job(rank, world, edit=two)
        parts = check_group_by(ctx, dx, up, mine, everything, ["s"], aggs, ["a", "b"], f"{name} two groups world {world}")
        assert sum(len(p) for p in parts) == 2
        if world > 1:  # rank 1 holds zero rows
            mine, everything, _ = job(rank, world, empty_rank=1)
            for key_names in (["s"], ["k2", "s"]):
                check_group_by(ctx, dx, up, mine, everything, key_names, aggs, ["a", "b"],
                               f"{name} rank 1 empty {key_names} world {world}")
    close(ctx, world)


def mode_window(rank, world):
    from qe_hip.plan import WindowFunctionType as W
    ctx, executors = setup(world)
    up = make_uploader(ctx)
    mine, everything, first = job(rank, world)
    n = len(mine["a"][0])
    for name, dx in executors:
        for part, order, asc in (("s", "a", True), ("k2", "s", False)):
            P, O, A = up(mine, part), up(mine, order), up(mine, "a")
            WP, WO, WA = up(everything, part), up(everything, order), up(everything, "a")
            cases = [
                ("row_number", lambda: dx.row_number([P], [O], [asc]), lambda: ctx.row_number([WP], [WO], [asc])),
                ("rank", lambda: dx.window(W.Rank, [P], [O], [asc]), lambda: ctx.window(W.Rank, [WP], [WO], [asc])),
                ("lag default", lambda: dx.window(W.Lag, [P], [O], [asc], arg=A, param=2, default=-7),
                 lambda: ctx.window(W.Lag, [WP], [WO], [asc], arg=WA, param=2, default=-7)),
                ("lag", lambda: dx.window(W.Lag, [P], [O], [asc], arg=A, param=2),
                 lambda: ctx.window(W.Lag, [WP], [WO], [asc], arg=WA, param=2)),
            ]
            for what, got_fn, want_fn in cases:
                got, want = got_fn(), want_fn()
                assert got.dtype == want.dtype and len(got) == n
                wv, wm = want.to_numpy()
                wm = np.ones(len(wv), bool) if wm is None else wm
                gv, gm = got.to_numpy()
                gm = np.ones(len(gv), bool) if gm is None else gm
                assert_col_equal((gv, gm), (wv[first:first + n], wm[first:first + n]),
                                 f"{name} {what} PARTITION BY {part} ORDER BY {order} world {world}")
                if what == "lag":
                    assert not wm.all()  # NULLs at the partition starts travel back
    close(ctx, world)


def mode_sort(rank, world):
    from qe_hip import abi
    ctx, executors = setup(world)
    up = make_uploader(ctx)

    def same(t):
        return dict(t, s10=(np.full(len(t["a"][0]), "日本", dtype=object), t["s10"][1]))

    def three(t):
        return dict(t, s10=(np.array(["ß", "", "straße"], dtype=object)[t["k2"][0] % 3], t["s10"][1]))

    def all_null(t):
        return dict(t, s10=(t["s10"][0], np.zeros(len(t["a"][0]), bool)))
    variants = [("base", None, None), ("one string", same, None), ("three strings", three, None), ("all NULL", all_null, None)]
    if world > 1:
        variants.append(("rank 1 empty", None, 1))
    for name, dx in executors:
        for vname, edit, empty_rank in variants:
            mine, everything, first = job(rank, world, empty_rank=empty_rank, edit=edit)
            n = len(mine["a"][0])
            mine["rowid"] = (np.arange(first, first + n, dtype=np.int64), None)
            everything["rowid"] = (np.arange(len(everything["a"][0]), dtype=np.int64), None)
            names = ["s10", "k2", "rowid"]
            for key_idx, asc in (([0], [True]), ([0, 1], [False, True])):
                what = f"{name} sort {vname} {key_idx} {asc} world {world}"
                out = dx.sort([up(mine, c) for c in names], key_idx, asc)
                assert [c.dtype for c in out] == [abi.DT_UTF8, abi.DT_INT64, abi.DT_INT64], what
                res = dx.gather_to_root(out)
                if rank == 0:
                    wcols = [up(everything, c) for c in names]
                    p = ctx.sort_indices([wcols[i] for i in key_idx], asc)
                    for j, c in enumerate(wcols):
                        wv, wm = ctx.take(c, p).to_numpy()
                        wm = np.ones(len(wv), bool) if wm is None else wm
                        assert_col_equal(res[j], (wv, wm), f"{what}: column {names[j]}")
    close(ctx, world)


def join_sides(q):
    """Rank q's sides: 2 000 build rows over 1 500 strings (duplicates, 5 % NULL) and 5 000 probe rows
    over 2 143 (about 30 % unmatched, 5 % NULL), each with a job-wide row id."""
    r = np.random.default_rng(1200 + q)
    name = lambda i: f"key-{int(i)}-é" if i % 2 else f"ключ-{int(i)}"  # noqa: E731
    bk = np.array([name(i) for i in r.integers(0, 1500, 2000)], dtype=object)
    pk = np.array([name(i) for i in r.integers(0, 2143, 5000)], dtype=object)
    return {"bk": (bk, r.random(2000) > 0.05), "bid": (np.arange(2000, dtype=np.int64) + 2000 * q, None)}, \
           {"pk": (pk, r.random(5000) > 0.05), "pid": (np.arange(5000, dtype=np.int64) + 5000 * q, None)}


def check_join(ctx, dx, P, B, WP, WB, what, local_join):
    op, ob, rows = dx.hash_join_inner(0, P, 0, B)
    assert all(len(c) == rows for c in op + ob), what
    assert [c.dtype for c in op + ob] == [c.dtype for c in P + B], (what, [c.dtype for c in op + ob])
    parts = [None] * dx.world
    dist.all_gather_object(parts, rows_of([c.to_numpy() for c in op + ob]))
    wp, wb, wrows = local_join(WP[0], WP, WB[0], WB)
    want = sorted(rows_of([c.to_numpy() for c in wp + wb]), key=row_key)
    got = sorted((t for part in parts for t in part), key=row_key)
    assert wrows == len(want) and wrows > 1000, (what, wrows)
    assert got == want, (what, len(got), len(want))
    # equal keys met on one rank
    owner = {}
    for q, part in enumerate(parts):
        for t in part:
            assert owner.setdefault(t[0], q) == q, (what, "a key joined on two ranks", t[0])


def mode_join(rank, world):
    ctx, executors = setup(world)
    sides = [join_sides(q) for q in range(world)]
    build, probe = sides[rank]
    wbuild, wprobe = concat([s[0] for s in sides]), concat([s[1] for s in sides])
    for name, dx in executors:
        P = [ctx.upload(*probe["pk"]), ctx.upload(*probe["pid"])]
        B = [ctx.upload(*build["bk"]), ctx.upload(*build["bid"])]
        WP = [ctx.upload(*wprobe["pk"]), ctx.upload(*wprobe["pid"])]
        WB = [ctx.upload(*wbuild["bk"]), ctx.upload(*wbuild["bid"])]
        check_join(ctx, dx, P, B, WP, WB, f"{name} Utf8 join world {world}",
                   lambda pk, pc, bk, bc: ctx.hash_join(0, pk, pc, bk, bc))
    close(ctx, world)


def mode_temporal(rank, world):
    from qe_hip import AggregateFunction as AF, abi
    from qe_hip.partition import DeviceBatch, Hash, Partitioner
    ctx, executors = setup(world)
    up = make_uploader(ctx)
    mine, everything, first = job(rank, world)
    n = len(mine["a"][0])
    aggs = [(AF.Sum, 0), (AF.Count, 0), (AF.Min, 0), (AF.Avg, 1)]
    for name, dx in executors:
        # GROUP BY a Date32 key and a Timestamp(us) key, NULL keys one group
        for key, dt in (("d32", abi.DT_DATE32), ("tus", abi.DT_TIMESTAMP_US)):
            parts = check_group_by(ctx, dx, up, mine, everything, [key], aggs, ["a", "b"],
                                   f"{name} group_by {key} world {world}", min_groups=41)
            assert any(t[0] is None for part in parts for t in part)
            keys, _, _ = dx.group_by([up(mine, key)], [up(mine, "a")], [(AF.Count, 0)])
            assert keys[0].dtype == dt
        # ORDER BY Timestamp(us) DESC (negative values, NULLs), a row id proving stability
        mine["rowid"] = (np.arange(first, first + n, dtype=np.int64), None)
        everything["rowid"] = (np.arange(len(everything["a"][0]), dtype=np.int64), None)
        out = dx.sort([up(mine, "tus"), up(mine, "rowid"), up(mine, "d32")], [0], [False])
        assert [c.dtype for c in out] == [abi.DT_TIMESTAMP_US, abi.DT_INT64, abi.DT_DATE32]
        res = dx.gather_to_root(out)
        if rank == 0:
            wcols = [up(everything, "tus"), up(everything, "rowid"), up(everything, "d32")]
            p = ctx.sort_indices([wcols[0]], [False])
            assert (everything["tus"][0] < 0).any()
            for j, c in enumerate(wcols):
                wv, wm = ctx.take(c, p).to_numpy()
                wm = np.ones(len(wv), bool) if wm is None else wm
                assert_col_equal(res[j], (wv, wm), f"{name} sort by Timestamp(us) DESC world {world}: column {j}")
        # ROW_NUMBER PARTITION BY Date32 ORDER BY Timestamp(ns)
        got = dx.row_number([up(mine, "d32")], [up(mine, "tns")], [True])
        wv, _ = ctx.row_number([up(everything, "d32")], [up(everything, "tns")], [True]).to_numpy()
        assert_col_equal((got.to_numpy()[0], None), (wv[first:first + n], None), f"{name} row_number world {world}")
        # join on Date64 keys
        pk = lambda t: [up(t, "d64"), up(t, "rowid")]  # noqa: E731
        r2 = [np.random.default_rng(1300 + q) for q in range(world)]
        bsides = [{"d64": (r.integers(-400, 400, 500).astype(np.int64) * 86_400_000, r.random(500) > 0.05),
                   "rowid": (np.arange(500, dtype=np.int64) + 500 * q, None)} for q, r in enumerate(r2)]
        check_join(ctx, dx, pk(mine), pk(bsides[rank]), pk(everything), pk(concat(bsides)),
                   f"{name} Date64 join world {world}", lambda a, b, c, d: ctx.hash_join_inner(a, b, c, d))
        # exchange by an Int64 key carrying Date32 and Timestamp(ms) payloads with NULLs
        names = ["k2", "a", "d32", "tms"]
        strat = Hash(["a"], world)
        got = dx.exchange(strat, DeviceBatch(names, [up(mine, c) for c in names]))
        assert [c.dtype for c in got.columns] == [abi.DT_INT64, abi.DT_INT64, abi.DT_DATE32, abi.DT_TIMESTAMP_MS]
        counts, moved = Partitioner(ctx, strat).batch_move(DeviceBatch(names, [up(everything, c) for c in names]))
        lo = int(np.sum(counts[:rank]))
        assert len(got.columns[0]) == int(counts[rank])
        for j, c in enumerate(moved):
            wv, wm = c.to_numpy()
            wm = np.ones(len(wv), bool) if wm is None else wm
            gv, gm = got.columns[j].to_numpy()
            gm = np.ones(len(gv), bool) if gm is None else gm
            assert_col_equal((gv, gm), (wv[lo:lo + len(gv)], wm[lo:lo + len(gv)]), f"{name} exchange world {world}: {names[j]}")
            if names[j] in ("d32", "tms"):
                assert not gm.all() or len(gm) == 0
    close(ctx, world)


def mode_refusals(rank, world):
    """What stays refused raises QEH_E_UNSUPPORTED on every rank, before any collective: a rank that
    raised alone, or after entering one, would leave the others waiting (the launcher's time limit).
    After each refusal the ranks run a collective operator together, which also shows they are in step."""
    from qe_hip import AggregateFunction as AF, abi
    from qe_hip.partition import DeviceBatch, Hash, Range
    ctx, executors = setup(world)
    up = make_uploader(ctx)
    mine, everything, _ = job(rank, world)
    aggs = [(AF.Count, 1)]
    for name, dx in executors:
        s, k2, a, d32, tus = (up(mine, c) for c in ("s", "k2", "a", "d32", "tus"))
        batch = DeviceBatch(["k2", "tus", "d32"], [k2, tus, d32])
        refused = [
            ("exchange by a temporal hash key", lambda: dx.exchange(Hash(["tus"], world), batch)),
            ("exchange by a temporal range key", lambda: dx.exchange(Range("d32", list(range(world - 1))), batch)),
            ("broadcast join on a Utf8 key", lambda: dx.join_filter_aggregate_broadcast([s, a], 0, None, s, [k2], aggs)),
            ("sharded broadcast join on a Utf8 key",
             lambda: dx.join_filter_aggregate_broadcast([k2, a], 0, None, s, [k2], aggs, build_sharded=True)),
            ("shuffle join on a Utf8 key", lambda: dx.join_filter_aggregate_shuffle([s, a], 0, None, s, [k2], aggs)),
        ]
        if world > 1:
            refused += [
                ("broadcast join grouped by a temporal key",
                 lambda: dx.join_filter_aggregate_broadcast([k2, a], 0, None, k2, [d32], aggs)),
                ("shuffle join grouped by a temporal key",
                 lambda: dx.join_filter_aggregate_shuffle([k2, a], 0, None, k2, [a, tus], aggs)),
                ("shuffle join on a temporal key", lambda: dx.join_filter_aggregate_shuffle([tus, a], 0, None, tus, [k2], aggs)),
                ("sharded broadcast join on a temporal key",
                 lambda: dx.join_filter_aggregate_broadcast([tus, a], 0, None, tus, [k2], aggs, build_sharded=True)),
            ]
        for what, fn in refused:
            try:
                fn()
            except abi.QehError as e:
                assert e.status == abi.QEH_E_UNSUPPORTED, (name, what, e.status, e.message)
            else:
                raise AssertionError(f"{name}: {what} was not refused")
            keys, out, g = dx.group_by([k2], [a], [(AF.Count, 0)])  # the ranks are still in step
            assert len(keys[0]) == g
        # Utf8 against a non-Utf8 join key stays the local type error, before a collective
        for P, B in (([s, a], [k2, a]), ([k2, a], [s, a]), ([d32, a], [tus, a])):
            try:
                dx.hash_join_inner(0, P, 0, B)
            except abi.QehError as e:
                assert e.status == abi.QEH_E_TYPE and "Invalid comparison operation" in e.message, (e.status, e.message)
            else:
                raise AssertionError("mismatched join keys were not refused")
            dx.group_by([k2], [a], [(AF.Count, 0)])
    close(ctx, world)


def main():
    mode = sys.argv[1]
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        {"group_by": mode_group_by, "window": mode_window, "sort": mode_sort, "join": mode_join,
         "temporal": mode_temporal, "refusals": mode_refusals}[mode](rank, world)
        dist.barrier()
    finally:
        dist.destroy_process_group()
    print(f"rank {rank} ok")


if __name__ == "__main__":
    main()
