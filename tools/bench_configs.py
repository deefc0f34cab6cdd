#!/usr/bin/env python3
"""Secondary BASELINE configs on one MI355X (the headline metric is bench.py).

  cfg2  Filter + GROUP BY SUM/COUNT: SELECT k, SUM(v), COUNT(v), SUM(vi) FROM t
        WHERE x > 49 GROUP BY k   (1e8 rows; 32 B/row algorithmic)
  cfg3  INNER hash join 1e9 x 1e7 materialising (f.v, d.a)
        (16 B probe + 16 B output per fact row; build 16 B/dim row)
  cfg5  ROW_NUMBER() OVER (PARTITION BY k ORDER BY v), k in [0, 2^20)
        (16 B read + 8 B write per row)
  filter  the Filter operator alone: SELECT x, k, v WHERE x > 49 (24 B in + 12 B out avg per row)
  limit   the same filter under LIMIT 1000 (capped filter, early exit)
  plan    the metric query through QueryExecutor from host Arrow batches, cold vs device-cached Scan
  left / full   LEFT / FULL outer join 2e8 x 1e7, half the probe rows unmatched
  merge   Merge::sorted of 8 partitions x 1.25e7 rows, ORDER BY k DESC NULLS LAST
  encode  pgwire DataRow text encoding of 1e7 result rows
  partition  device side of a hash Exchange, 1e8 rows into 8 partitions
  cfg5leg    config 5's per-rank device leg at N = 8 (8-way exchange pass, local ROW_NUMBER over the
             received rows, the unmove pass that returns the numbers to input order)
  utf8_groupby  GROUP BY a Utf8 key: 1e8 rows over 1024 distinct strings of 8-24 bytes, COUNT + SUM of an
             Int64 column; beside it the same query over the pre-encoded Int32 codes and the
             dictionary encode alone against its floor (offsets + string bytes read, codes written)
  utf8_sort  ORDER BY a Utf8 key: 1e8 rows of all-distinct 16-byte strings; same companions
  utf8_join  INNER JOIN on a Utf8 key: 1e8 probe rows against 1e6 distinct build strings of 8-24 bytes, 10 %
             of the probe rows absent; the shared-dictionary encode split into insert and lookup, the lookup
             against its floor, and the same join over codes encoded ahead of time
  topk       ORDER BY k LIMIT 100 over 1e8 rows (spread Int64, Float64, Int64 in [0, 1024)): the radix-select
             path of qeh_sort_indices_limit against the full sort in the same process, then the limit / n, n and
             candidate-share sweeps behind its fallback constants
  semi       k IN (set) through qeh_in_set: 1e9 Int64 probe keys against a dense 1e7-key set (bitmap form) and
             1e8 probe keys against 1e7 sparse 64-bit keys (hash-set form); beside each the byte floor (8 B
             read + 1 bit written per row at 8 TB/s) and the closest operator there was before,
             hash_join_inner of the same probe against the same (distinct) set emitting the probe key only
  tsmatch    to_tsvector(doc) @@ to_tsquery('gpu & kernel') over 1e7 documents of about 64 bytes: the stream
             kernel against the row-per-lane kernel (QEH_NO_TS_STREAM=1), interleaved, with GB/s over the
             bytes read
  csv        qeh_scan_csv over 1e7 rows x (Int64, Float64 as shortest repr, Utf8 of 4-12 bytes, Date32): wall and
             kernel time with the bytes on the device and with the upload included, the share of Float64 cells
             parsed on the host, the byte floor (the file read by each pass plus the columns written, at 8 TB/s),
             and pyarrow.csv.read_csv of the same bytes on 16 threads (the stand-in for arrow-csv)
  cfg4leg    config 4's per-rank device leg at N = 8 (fused filter + 8-way exchange pass over 1e9
             rows, the dim shard's exchange pass, the local join of what the rank receives)

Prints one JSON line per config: rows/s, ms per run, algorithmic GB/s and
fraction of 8 TB/s, and the oracle's rows/s on a bounded sample (1 thread).
usage: python tools/bench_configs.py [--only cfg2,cfg3,cfg5,window,filter,limit,plan,left,full,merge,encode,partition,utf8_groupby,utf8_sort,utf8_join,topk,semi,tsmatch,temporal,csv] [--scale 1.0]
"""
import argparse
import json
import os
import re
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "query-engine_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (one HIP runtime: torch first, see qe_hip/abi.py)

import qe_hip  # noqa: E402
import oracle_bind as ob  # noqa: E402
from qe_hip import AggregateFunction as AF, BinaryOp, abi, binop, col, lit  # noqa: E402

PEAK = 8000.0
SEED = 0x5EED


def timed(ctx, fn, reps, names):
    fn()
    ctx.sync()
    ctx.timing(True)
    ctx.timing_reset()
    t0 = time.perf_counter()
    for _ in range(reps):
        out = fn()
    ctx.sync()
    wall = (time.perf_counter() - t0) / reps
    kt = {n: ctx.kernel_time(n)[0] / reps for n in names}
    ctx.timing(False)
    return wall, kt, out


def line(cfg, rows, wall, alg_bytes, kernel_ms, kernel, cpu, extra=None):
    gbs = alg_bytes / (kernel_ms * 1e-3) / 1e9 if kernel_ms and alg_bytes else None
    d = {"config": cfg, "rows": rows, "rows_per_s": rows / wall, "ms_per_run": wall * 1e3,
         "dominant_kernel": kernel, "kernel_ms": kernel_ms, "alg_bytes": alg_bytes,
         "achieved_GBs": gbs, "frac_of_8TBs": gbs / PEAK if gbs else None, "cpu_baseline": cpu}
    if extra:
        d.update(extra)
    print(json.dumps(d), flush=True)


def cfg2(ctx, scale):
    n = int(1e8 * scale)
    x = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 1, n, 100)
    k = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 2, n, 1024)
    v = ctx.generate(abi.GEN_UNIT_F64, SEED, 3, n)
    vi = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 4, n, 2 ** 21, lo=-(2 ** 20))
    pred = binop(col(0), BinaryOp.Greater, lit(49))
    fn = lambda: ctx.filter_aggregate([x, k, v, vi], pred, [1], [(AF.Sum, 2), (AF.Count, 2), (AF.Sum, 3)])
    wall, kt, _ = timed(ctx, fn, 10, ["aggregate_rows", "group_insert"])
    m = 20_000_000
    hx = ob.generate(abi.GEN_UNIFORM_MOD, SEED, 1, m, 100)
    hk = ob.generate(abi.GEN_UNIFORM_MOD, SEED, 2, m, 1024)
    hv = ob.generate(abi.GEN_UNIT_F64, SEED, 3, m)
    hvi = ob.generate(abi.GEN_UNIFORM_MOD, SEED, 4, m, 2 ** 21, lo=-(2 ** 20))
    t0 = time.perf_counter()
    fc, rows, _ = ob.filter([ob.HostCol(hx), ob.HostCol(hk), ob.HostCol(hv), ob.HostCol(hvi)], pred)
    fh = [ob.HostCol(a, b) for a, b in fc]
    ob.hash_aggregate([fh[1]], fh, [(AF.Sum, 2), (AF.Count, 2), (AF.Sum, 3)])
    dt = time.perf_counter() - t0
    cpu = {"value": m / dt, "unit": "rows/s", "cores": 1, "kind": "port", "sample": f"{m} rows, {dt:.2f} s"}
    kms = kt["aggregate_rows"] + kt["group_insert"]
    line("cfg2 filter+group-by 1e8", n, wall, 32.0 * n, kms, "k_group_agg_fast (LDS key hash per workgroup)", cpu)


def cfg3(ctx, scale):
    n, nd = int(1e9 * scale), 10_000_000
    fk = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 2, n, nd)
    fv = ctx.generate(abi.GEN_UNIT_F64, SEED, 3, n)
    dk = ctx.generate(abi.GEN_PERMUTATION, SEED, 0, nd, nd)
    da = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 6, nd, 1000)

    def fn():
        p, b, rows = ctx.hash_join_inner(fk, [fv], dk, [da])
        for c in p + b:
            c.release()
        return rows
    wall, kt, rows = timed(ctx, fn, 3, ["join_probe", "join_gather", "join_build"])
    m = 20_000_000
    hk = ob.generate(abi.GEN_UNIFORM_MOD, SEED, 2, m, nd)
    hv = ob.generate(abi.GEN_UNIT_F64, SEED, 3, m)
    hdk = ob.generate(abi.GEN_PERMUTATION, SEED, 0, nd, nd)
    hda = ob.generate(abi.GEN_UNIFORM_MOD, SEED, 6, nd, 1000)
    t0 = time.perf_counter()
    ob.hash_join_inner(ob.HostCol(hk), [ob.HostCol(hv)], ob.HostCol(hdk), [ob.HostCol(hda)])
    dt = time.perf_counter() - t0
    cpu = {"value": m / dt, "unit": "rows/s", "cores": 1, "kind": "port", "sample": f"{m} probe x {nd} build, {dt:.2f} s"}
    kms = kt["join_probe"] + kt["join_gather"]
    line("cfg3 inner join 1e9 x 1e7", n, wall, 32.0 * n, kms, "k_slice_count + k_slice_partition + k_slice_join_inplace", cpu,
         {"output_rows": rows, "build_ms": kt["join_build"]})


def cfg3_wide(ctx, scale):
    """cfg3 with a full-range Int64 build payload: the u16 frame-of-reference of the slice path
    does not apply, so the fused embedded-record join (k_join_mat) runs."""
    n, nd = int(1e9 * scale), 10_000_000
    fk = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 2, n, nd)
    fv = ctx.generate(abi.GEN_UNIT_F64, SEED, 3, n)
    dk = ctx.generate(abi.GEN_PERMUTATION, SEED, 0, nd, nd)
    da = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 6, nd, 1 << 62)

    def fn():
        p, b, rows = ctx.hash_join_inner(fk, [fv], dk, [da])
        for c in p + b:
            c.release()
        return rows
    wall, kt, rows = timed(ctx, fn, 3, ["join_probe", "join_gather", "join_build", "join_mat"])
    line("cfg3 inner join 1e9 x 1e7, full-range Int64 payload", n, wall, 32.0 * n, wall * 1e3,
         "k_join_mat (embedded build records)", None, {"output_rows": rows, "kernel_split_ms": kt,
                                                         "note": "kernel_ms = wall: the path has no single timer"})


def cfg_metric_shapes(ctx, scale, only=("sparse", "g17", "agg2")):
    """The metric query beyond the dense-key best case (1e9 fact rows x 1e7 dim rows):
      sparse  dim keys are sparse 64-bit values (H(i), GEN_SPARSE_KEY), fact keys drawn from them
      g17     2^17 groups (d.g uniform in [0, 2^17))
      agg2    two aggregate columns: SUM(f.v), SUM(f.w), COUNT(f.v)
    Algorithmic bytes: 24 B per fact row (x, k, v; +8 B for w) + 16 B per dim row."""
    n, nd = int(1e9 * scale), 10_000_000
    x = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 1, n, 100)
    v = ctx.generate(abi.GEN_UNIT_F64, SEED, 3, n)
    pred = binop(col(0), BinaryOp.Greater, lit(49))
    names = ["join_filter_aggregate", "slice_partition", "slice_probe", "slice_keyagg", "join_build", "aggregate_rows"]
    for shape in only:
        if shape == "sparse":
            k = ctx.generate(abi.GEN_SPARSE_KEY, SEED, 2, n, nd)
            dk = ctx.generate(abi.GEN_SPARSE_KEY, SEED, 0, nd, 0)
            dg = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 5, nd, 1024)
            cols, aggs, alg = [x, k, v], [(AF.Sum, 2), (AF.Count, 2)], 24.0
        elif shape == "g17":
            k = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 2, n, nd)
            dk = ctx.generate(abi.GEN_PERMUTATION, SEED, 0, nd, nd)
            dg = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 5, nd, 1 << 17)
            cols, aggs, alg = [x, k, v], [(AF.Sum, 2), (AF.Count, 2)], 24.0
        else:
            k = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 2, n, nd)
            dk = ctx.generate(abi.GEN_PERMUTATION, SEED, 0, nd, nd)
            dg = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 5, nd, 1024)
            w = ctx.generate(abi.GEN_UNIT_F64, SEED, 9, n)
            cols, aggs, alg = [x, k, v, w], [(AF.Sum, 2), (AF.Sum, 3), (AF.Count, 2)], 32.0

        def fn():
            gk, ga, g = ctx.join_filter_aggregate(cols, 1, pred, dk, [dg], aggs)
            for c in gk + ga:
                c.release()
            return g
        wall, kt, g = timed(ctx, fn, 5, names)
        # the slice pipeline ran when phase A holds a real share of the wall time (a declined prelaunch
        # leaves a few microseconds on its timers: r04's sparse line summed those, frac 184)
        sliced = kt["slice_partition"] > 0.1 * wall * 1e3
        kms = kt["slice_partition"] + kt["slice_probe"] + kt["slice_keyagg"] if sliced else kt["join_filter_aggregate"]
        dom = ("k_slice_partition + k_slice_keyagg" if kt["slice_keyagg"] else "k_slice_partition + k_slice_probe") \
            if sliced else "single pass (join_filter_aggregate)"
        line(f"metric shape {shape} 1e9 x 1e7", n, wall, alg * n + 16.0 * nd, kms, dom,
             None, {"groups": g, "kernel_split_ms": kt})
        del k, dk, dg


def cfg5(ctx, scale):
    n = int(1e9 * scale)
    k = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 7, n, 2 ** 20)
    v = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 8, n, 2 ** 62, lo=-(2 ** 61))

    def fn():
        rn = ctx.row_number([k], [v], [True])
        rn.release()
    wall, kt, _ = timed(ctx, fn, 2, ["radix_pass", "sort_encode", "row_number", "window_partition", "window_sort", "window_place",
                                    "w3_partition", "w3_sort", "w3_place"])
    m = 5_000_000
    hk = ob.generate(abi.GEN_UNIFORM_MOD, SEED, 7, m, 2 ** 20)
    hv = ob.generate(abi.GEN_UNIFORM_MOD, SEED, 8, m, 2 ** 62, lo=-(2 ** 61))
    t0 = time.perf_counter()
    ob.row_number([ob.HostCol(hk)], [ob.HostCol(hv)], [True])
    dt = time.perf_counter() - t0
    cpu = {"value": m / dt, "unit": "rows/s", "cores": 1, "kind": "port", "sample": f"{m} rows, {dt:.2f} s"}
    kms = sum(kt.values())
    line("cfg5 ROW_NUMBER 1e9", n, wall, 24.0 * n, kms, "k_window.hip partition passes + wave sort + placement (LSD sort fallback)", cpu, kt)


def cfg_window(ctx, scale):
    """RANK() and LAG(v, 1) OVER (PARTITION BY k ORDER BY v) on the cfg-5 data (1e9 rows)."""
    from qe_hip.plan import WindowFunctionType as W
    n = int(1e9 * scale)
    k = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 7, n, 2 ** 20)
    v = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 8, n, 2 ** 62, lo=-(2 ** 61))
    m = 2_000_000
    hk = ob.generate(abi.GEN_UNIFORM_MOD, SEED, 7, m, 2 ** 20)
    hv = ob.generate(abi.GEN_UNIFORM_MOD, SEED, 8, m, 2 ** 62, lo=-(2 ** 61))
    for name, func, arg, alg in [("RANK", W.Rank, None, 24.0), ("LAG(v,1)", W.Lag, v, 24.0)]:
        def fn():
            ctx.window(func, [k], [v], [True], arg=arg, param=1).release()
        wall, kt, _ = timed(ctx, fn, 2, ["radix_pass", "sort_encode", "window", "window_partition", "window_sort", "window_place", "w3_partition", "w3_sort", "w3_place"])
        t0 = time.perf_counter()
        ob.window(func, [ob.HostCol(hk)], [ob.HostCol(hv)], [True], arg=ob.HostCol(hv) if arg is not None else None,
                  param=1)
        dt = time.perf_counter() - t0
        cpu = {"value": m / dt, "unit": "rows/s", "cores": 1, "kind": "port", "sample": f"{m} rows, {dt:.2f} s"}
        line(f"window {name} 1e9", n, wall, alg * n, sum(kt.values()), "radix sort + k_seg_start/k_window_out", cpu, kt)


def cfg_window_lsd(ctx, scale):
    """Window shapes beyond config 5's: ROW_NUMBER() and RANK() OVER (PARTITION BY k ORDER BY v) with k
    over 2^24 values (groups of 16 consecutive keys in the partitioning path), and ROW_NUMBER over two
    PARTITION BY keys (64 x 2^16 values: their composite key takes the same path), 1e9 rows.
    QEH_WM_NO_SUB=1 / QEH_NO_WINDOW_MSD=1 give the LSD path for comparison.  Algorithmic bytes: 16 B read
    + 8 B written per row (24 B read with the second key)."""
    from qe_hip.plan import WindowFunctionType as W
    n = int(1e9 * scale)
    k = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 7, n, 2 ** 24)
    v = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 8, n, 2 ** 62, lo=-(2 ** 61))
    names = ["radix_pass", "sort_encode", "row_number", "window", "window_partition", "window_sort", "window_place", "gather",
             "w3_partition", "w3_sort", "w3_place"]
    for label, fn, alg in [
            ("ROW_NUMBER, k over 2^24", lambda: ctx.row_number([k], [v], [True]).release(), 24.0),
            ("RANK, k over 2^24", lambda: ctx.window(W.Rank, [k], [v], [True]).release(), 24.0)]:
        wall, kt, _ = timed(ctx, fn, 2, names)
        path = "partitioning path" if kt["window_sort"] else "LSD path"
        line(f"window {label} 1e9 ({path})", n, wall, alg * n, sum(kt.values()), path, None,
             {"kernel_split_ms": {q: w for q, w in kt.items() if w}})
    k2 = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 9, n, 64)
    kk = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 7, n, 2 ** 16)
    wall, kt, _ = timed(ctx, lambda: ctx.row_number([kk, k2], [v], [True]).release(), 2, names)
    path = "partitioning path, composite key" if kt["window_sort"] else "LSD path"
    line(f"window ROW_NUMBER, PARTITION BY (k, k2) 1e9 ({path})", n, wall, 32.0 * n, sum(kt.values()), path, None,
         {"kernel_split_ms": {q: w for q, w in kt.items() if w}})


def cfg_outer(ctx, scale, jt=1):
    """LEFT (jt=1) / FULL (jt=3) join, 2e8 probe rows (keys uniform over twice the dim key range,
    so half find no match) x 1e7 dim rows, materialising (f.v, d.a).  Algorithmic bytes: 16 B probe
    read + 16 B output written per output row (+ the FULL tail)."""
    n, nd = int(2e8 * scale), 10_000_000
    fk = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 2, n, 2 * nd)
    fv = ctx.generate(abi.GEN_UNIT_F64, SEED, 3, n)
    dk = ctx.generate(abi.GEN_PERMUTATION, SEED, 0, nd, nd)
    da = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 6, nd, 1000)

    def fn():
        lo, ro, rows = ctx.hash_join_outer(jt, fk, [fk, fv], dk, [da])
        for c in lo + ro:
            c.release()
        return rows
    wall, kt, rows = timed(ctx, fn, 5, ["join_probe", "join_count", "join_gather", "join_build"])
    m = 10_000_000
    hk = ob.generate(abi.GEN_UNIFORM_MOD, SEED, 2, m, 2 * nd)
    hv = ob.generate(abi.GEN_UNIT_F64, SEED, 3, m)
    hdk = ob.generate(abi.GEN_PERMUTATION, SEED, 0, nd, nd)
    hda = ob.generate(abi.GEN_UNIFORM_MOD, SEED, 6, nd, 1000)
    t0 = time.perf_counter()
    ob.hash_join_outer(jt, ob.HostCol(hk), [ob.HostCol(hk), ob.HostCol(hv)], ob.HostCol(hdk), [ob.HostCol(hda)])
    dt = time.perf_counter() - t0
    cpu = {"value": m / dt, "unit": "rows/s", "cores": 1, "kind": "port", "sample": f"{m} probe x {nd} build, {dt:.2f} s"}
    kms = kt["join_probe"] + kt["join_count"] + kt["join_gather"]
    name = {1: "LEFT", 3: "FULL"}[jt]
    # LEFT over the unique dim takes the embedded path: probe payloads leave as views, so only the
    # key is read and the build column (+ validity) written; FULL gathers every output column
    alg = 16.0 * n + n / 8 if jt == 1 else 16.0 * n + 24.0 * rows
    line(f"{name} outer join 2e8 x 1e7 (50% unmatched)", n, wall, alg, kms,
         "order-preserving slice probe k_os_part + k_os_probe + k_os_emit (FULL: + unmatched build rows)", cpu, {"output_rows": rows, "kernel_split_ms": kt})


def cfg_merge(ctx, scale):
    """Merge::sorted of 8 partitions x 1.25e7 rows (k Int64 with 5 % NULLs, v Float64), ORDER BY k
    DESC NULLS LAST.  Algorithmic bytes: read 16 B + write 16 B per row (+ validity)."""
    parts = []
    per = int(1.25e7 * scale)
    for p in range(8):
        k = ctx.generate(abi.GEN_UNIFORM_MOD, SEED + p, 7, per, 2 ** 40)
        kv, _ = k.to_numpy()
        valid = np.random.default_rng(p).random(per) > 0.05
        parts.append([ctx.upload(kv, valid), ctx.generate(abi.GEN_UNIT_F64, SEED + p, 8, per)])
    n = 8 * per

    def fn():
        cols, rows = ctx.merge_sorted(parts, [0], [False], [False])
        for c in cols:
            c.release()
        return rows
    wall, kt, rows = timed(ctx, fn, 3, ["merge_concat", "radix_pass", "sort_encode", "gather"])
    hk = [p[0].to_numpy() for p in parts]
    m = 4_000_000
    hkk = np.concatenate([a for a, _ in hk])[:m]
    hkv = np.concatenate([b for _, b in hk])[:m]
    t0 = time.perf_counter()
    ob.sort_indices_nulls([ob.HostCol(hkk, hkv)], [False], [False])
    dt = time.perf_counter() - t0
    cpu = {"value": m / dt, "unit": "rows/s", "cores": 1, "kind": "port", "sample": f"{m} rows sort, {dt:.2f} s"}
    line("Merge::sorted 8 x 1.25e7 rows, ORDER BY k DESC NULLS LAST", n, wall, 32.0 * n, sum(kt.values()),
         "k_rs_hist/k_rs_scatter carrying the payload (encode on load in pass 0, decode on store in the last)", cpu, kt)


def cfg_encode(ctx, scale):
    """§8 f4: pgwire DataRow text encoding of a 1e7-row result (k Int64, sum Float64, count Int64),
    the shape of the metric query's output rows at scale.  Bytes: 24 B read per row + the encoded
    messages written."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import pg_text
    n = int(1e7 * scale)
    k = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 2, n, 1 << 40)
    v = ctx.generate(abi.GEN_UNIT_F64, SEED, 3, n)
    c = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 4, n, 1000000)

    def fn():
        out = ctx.encode_pg_datarows([k, v, c])
        nb = out.c.values_bytes
        out.release()
        return nb
    wall, kt, nbytes = timed(ctx, fn, 5, ["encode_len", "encode_write"])
    m = 100_000
    hk, hv, hc = (x.to_numpy()[0][:m] for x in (k, v, c))
    t0 = time.perf_counter()
    pg_text.encode_rows([("int64", hk.tolist()), ("float64", hv.tolist()), ("int64", hc.tolist())])
    dt = time.perf_counter() - t0
    cpu = {"value": m / dt, "unit": "rows/s", "cores": 1, "kind": "port",
           "sample": f"{m} rows, oracle/pg_text.py (pure Python), {dt:.2f} s"}
    line("pgwire DataRow text encoding 1e7 x (Int64, Float64, Int64)", n, wall, 24.0 * n + nbytes,
         sum(kt.values()), "k_pg_row_len + k_pg_row_write (Schubfach shortest floats)", cpu,
         {"encoded_bytes": nbytes, "kernel_split_ms": kt})
    # Arrow IPC stream of the same batch (network.rs:56-72): device normalisation + copy to host
    reps = 5
    data = ctx.encode_arrow_ipc([k, v, c], ["k", "sum", "count"])
    t0 = time.perf_counter()
    for _ in range(reps):
        data = ctx.encode_arrow_ipc([k, v, c], ["k", "sum", "count"])
    wall = (time.perf_counter() - t0) / reps
    names, cols, _ = ctx.decode_arrow_ipc(data)
    t0 = time.perf_counter()
    for _ in range(reps):
        names, cols, _ = ctx.decode_arrow_ipc(data)
        for x in cols:
            x.release()
    wall_d = (time.perf_counter() - t0) / reps
    line("Arrow IPC stream encode 1e7 x (Int64, Float64, Int64), device -> host bytes", n, wall, None, None,
         "device normalise + D2H copies", None,
         {"stream_bytes": len(data), "host_GBs": len(data) / wall / 1e9, "decode_ms": wall_d * 1e3,
          "decode_host_GBs": len(data) / wall_d / 1e9})


def cfg_partition(ctx, scale):
    """§8 f2: the device side of a hash Exchange into 8 partitions (one per GPU of a node):
    1e8 rows x (k Int64, v Float64) -> partition-major columns + counts.  Bytes: 16 B read +
    16 B written per row (the permutation is an intermediate)."""
    from qe_hip.partition import DeviceBatch, Hash, Partitioner
    n = int(1e8 * scale)
    k = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 2, n, 1 << 40)
    v = ctx.generate(abi.GEN_UNIT_F64, SEED, 3, n)
    pt = Partitioner(ctx, Hash(["k"], 8))
    b = DeviceBatch(["k", "v"], [k, v])

    def fn():
        counts, moved = pt.batch_move(b)
        for c in moved:
            c.release()
        return counts
    wall, kt, counts = timed(ctx, fn, 5, ["partition_move"])
    line("hash Exchange 1e8 rows x (Int64, Float64) into 8 partitions (device side)", n, wall, 32.0 * n,
         sum(kt.values()), "k_hash_ids8 + k_rs_hist + k_part_scatter (columns moved in one pass)", None,
         {"kernel_split_ms": kt, "max_partition_share": float(max(counts)) / n})


def cfg4_leg(ctx, scale, world=8):
    """BASELINE config 4's per-rank device leg at N = 8, on one GPU: what one rank of the
    hash-partitioned plan runs besides the RCCL all-to-all (DistributedExecutor.
    join_filter_aggregate_shuffle; partition.rs:151-212, planner.rs:200-249):
      1. filter f.x > 49 fused into the 8-way hash exchange pass over its 1e9 fact rows
         (qeh_filter_partition_hash_move: x, k, v read once, (k, v) of the selected rows written
         partition-major);
      2. the 8-way hash exchange pass over its dim shard (1e7 / 8 rows of (k, g));
      3. the local fused join + partial aggregate over what the rank receives: the rows of ITS
         partition from all 8 ranks — stood in for by 8 copies of this rank's partition 0 (same
         size and key distribution: uniform keys send 1/8 of every rank's rows to each rank) —
         against the dim keys of partition 0 (a sparse 1/8 of the key range).
    Algorithmic bytes: 24 B read + 16 B written per selected row in (1), 32 B per dim row in (2),
    16 B per received row in (3)."""
    from qe_hip.partition import DeviceBatch  # noqa: F401  (same package the plan uses)
    n, nd = int(1e9 * scale), 10_000_000
    x = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 1, n, 100)
    k = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 2, n, nd)
    v = ctx.generate(abi.GEN_UNIT_F64, SEED, 3, n)
    dn = nd // world
    dk = ctx.generate(abi.GEN_PERMUTATION, SEED, 0, dn, nd)
    dg = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 5, dn, 1024)
    pred = binop(col(0), BinaryOp.Greater, lit(49))
    aggs = [(AF.Sum, 1), (AF.Count, 1)]
    # what rank 0 receives (built once, outside the timed legs)
    pc, pm = ctx.filter_partition_hash_move([x, k, v], pred, 1, world, [1, 2])
    selected = int(pc.sum())
    recv_k = ctx.concat([ctx.slice(pm[0], 0, int(pc[0]))] * world)
    recv_v = ctx.concat([ctx.slice(pm[1], 0, int(pc[0]))] * world)
    for c in pm:
        c.release()
    full_dk = ctx.generate(abi.GEN_PERMUTATION, SEED, 0, nd, nd)
    full_dg = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 5, nd, 1024)
    bc, bm = ctx.partition_hash_move([full_dk], world, [full_dk, full_dg])
    bk0, bg0 = ctx.slice(bm[0], 0, int(bc[0])), ctx.slice(bm[1], 0, int(bc[0]))
    recv = len(recv_k)

    def leg1():
        c, m = ctx.filter_partition_hash_move([x, k, v], pred, 1, world, [1, 2])
        for q in m:
            q.release()
        return c

    def leg2():
        c, m = ctx.partition_hash_move([dk], world, [dk, dg])
        for q in m:
            q.release()
        return c

    def leg3():
        gk, ga, g = ctx.join_filter_aggregate([recv_k, recv_v], 0, None, bk0, [bg0], aggs)
        for q in gk + ga:
            q.release()
        return g
    names = ["partition_move", "filter", "join_filter_aggregate", "slice_partition", "slice_probe", "join_build"]
    w1, k1, _ = timed(ctx, leg1, 5, names)
    w2, k2, _ = timed(ctx, leg2, 5, names)
    w3, k3, g = timed(ctx, leg3, 5, names)
    # bytes each leg moves through HBM (intermediates included: the exchange's writes and re-reads)
    b1, b2, b3 = 24.0 * n + 16.0 * selected, 32.0 * dn, 16.0 * recv
    kms1 = k1["partition_move"] + k1["filter"]
    kms3 = k3["slice_partition"] + k3["slice_probe"] if k3["slice_partition"] else k3["join_filter_aggregate"]
    legs = {"exchange_pass_fact": {"ms": kms1, "wall_ms": w1 * 1e3, "hbm_bytes_moved": b1,
                                   "moved_GBs": b1 / (kms1 * 1e-3) / 1e9},
            "exchange_pass_dim": {"ms": k2["partition_move"], "wall_ms": w2 * 1e3, "hbm_bytes_moved": b2},
            "local_join": {"ms": kms3, "wall_ms": w3 * 1e3, "hbm_bytes_moved": b3, "rows": recv, "groups": g,
                           "build_ms": k3["join_build"], "kernels": "slice" if k3["slice_partition"] else "single pass",
                           "moved_GBs": b3 / (kms3 * 1e-3) / 1e9}}
    kms = kms1 + k2["partition_move"] + kms3
    # the per-GPU algorithmic bytes of config 4 are the metric's (24 B per fact row
    # + 16 B per dim row read once, intermediates excluded); the exchange is reported separately
    alg = 24.0 * n + 16.0 * nd
    xgmi = (world - 1) / world * (16.0 * selected + 16.0 * dn)
    line(f"cfg4 per-rank device leg at N={world} (1e9 fact rows + 1/{world} dim per rank)", n, w1 + w2 + w3,
         alg, kms, "k_hash_ids8_pred + k_part_scatter (fused filter + 8-way exchange), local fused join",
         None, {"legs": legs, "selected": selected, "exchange_hbm_bytes": b1 + b2 + b3 - 24.0 * n - 16.0 * dn,
                "xgmi_bytes_per_rank": xgmi,
                "note": "frac on SURVEY §8(d)'s 24 B / fact row + 16 B / dim row; the exchange's HBM writes and "
                        "re-reads are in exchange_hbm_bytes, the bytes leaving the rank over xGMI in "
                        "xgmi_bytes_per_rank; RCCL all-to-all time excluded (8-GPU runs are the driver's); "
                        "wall = sum of the legs"})


def cfg4_items_leg(ctx, scale, world=8, rank=5):
    """BASELINE config 4's per-rank device leg at N = 8 in the shuffle join's items form
    (DistributedExecutor._shuffle_items, include/qeh.h qeh_shuffle_items_*), on one GPU: rank `rank`'s
    phase A over its 1e9 fact rows with the regions laid out per destination, its 1/8 of the dimension
    grouped by slice (k_dim_items), the per-destination packing, and phase B over what it receives --
    stood in for by its own block for itself from each of the 8 sources (uniform keys send every rank
    the same share) -- against its slices, built from the whole dimension's items (the all-gather's
    result).  RCCL time excluded (8-GPU runs are the driver's).  Algorithmic bytes as cfg4leg."""
    import torch
    from qe_hip.distributed import _DeviceView
    n, nd = int(1e9 * scale), 10_000_000
    x = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 1, n, 100)
    k = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 2, n, nd)
    v = ctx.generate(abi.GEN_UNIT_F64, SEED, 3, n)
    full_dk = ctx.generate(abi.GEN_PERMUTATION, SEED, 0, nd, nd)
    full_dg = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 5, nd, 1024)
    b = np.linspace(0, nd, world + 1).astype(int)
    shards = [(ctx.slice(full_dk, int(b[r]), int(b[r + 1] - b[r])), ctx.slice(full_dg, int(b[r]), int(b[r + 1] - b[r])))
              for r in range(world)]
    pred = binop(col(0), BinaryOp.Greater, lit(49))
    aggs = [(AF.Sum, 2), (AF.Count, 2)]
    row_len = 7
    rows = []
    for dk, dg in shards:
        row = torch.empty(row_len, dtype=torch.int64, device="cuda")
        ctx.broadcast_stats(dk, dg, [0, 1], row.data_ptr())
        rows.append(row)
    M = torch.cat(rows)
    ctx.sync()
    G = 1024
    nb, span = ctx.fused_items_shape(int(np.diff(b).max()), world)
    OW = 2 * 161
    # every shard's dimension items once (the all-gather's result), from throwaway handles
    gi = torch.empty(world * nb * span, dtype=torch.int32, device="cuda")
    go = torch.empty(world * nb * OW, dtype=torch.int32, device="cuda")
    tiny = [ctx.slice(x, 0, 8192), ctx.slice(k, 0, 8192), ctx.slice(v, 0, 8192)]
    for r, (dk, dg) in enumerate(shards):
        h = ctx.shuffle_items_begin(tiny, 1, pred, aggs, M.data_ptr(), world, r, row_len)
        ctx.fused_items_build(h, dk, dg, nb, span, gi.data_ptr() + r * nb * span * 4, go.data_ptr() + r * nb * OW * 4)
        ctx.fused_items_abort(h)
    ctx.sync()
    names = ["slice_partition", "shuffle_pack", "slice_probe", "fused_build"]
    nl = (1 + len(aggs)) * G + 1
    lanes = torch.empty(nl, dtype=torch.float64, device="cuda")
    best = None
    for rep in range(4):
        ctx.timing(True)
        ctx.timing_reset()
        t0 = time.perf_counter()
        h = ctx.shuffle_items_begin([x, k, v], 1, pred, aggs, M.data_ptr(), world, rank, row_len)
        it = torch.empty(nb * span, dtype=torch.int32, device="cuda")
        of = torch.empty(nb * OW, dtype=torch.int32, device="cuda")
        dk, dg = shards[rank]
        ctx.fused_items_build(h, dk, dg, nb, span, it.data_ptr(), of.data_ptr())
        ok, kp, vp, cp, bc, E, tot = ctx.shuffle_items_pack(h, world)
        assert ok
        # the receive buffers' stand-in: a packed block of this rank's (the next rank's, same size under
        # uniform keys) once per remote source; its own block is read in place by phase B
        kt = torch.as_tensor(_DeviceView(kp, world * bc, "<i2", None))
        vt = torch.as_tensor(_DeviceView(vp, world * bc, "<i8", None))
        ct = torch.as_tensor(_DeviceView(cp, world * E, "<i4", None))
        q1 = (rank + 1) % world
        t1 = int(tot[q1])
        rk = torch.cat([kt[q1 * bc:q1 * bc + t1]] * (world - 1) + [torch.zeros(4, dtype=torch.int16, device="cuda")])
        rv = torch.cat([vt[q1 * bc:q1 * bc + t1]] * (world - 1) + [torch.zeros(4, dtype=torch.int64, device="cuda")])
        rc = torch.cat([ct[q1 * E:(q1 + 1) * E] if q != rank else ct[rank * E:(rank + 1) * E] for q in range(world)])
        so, off = [], 0
        for q in range(world):
            so.append(off)
            off += t1 if q != rank else 0
        ctx.shuffle_items_finish(h, rk.data_ptr(), rv.data_ptr(), rc.data_ptr(), so, gi.data_ptr(), span, go.data_ptr(),
                                 world * nb, G, lanes.data_ptr())
        ctx.sync()
        wall = time.perf_counter() - t0
        kt_ = {nm: ctx.kernel_time(nm)[0] for nm in names}
        ctx.timing(False)
        if rep and (best is None or sum(kt_.values()) < sum(best[1].values())):
            best = (wall, kt_, int(tot.sum()), t1 * (world - 1) + int(tot[rank]))
        del rk, rv, rc
    wall, kt_, sent, recv = best
    kms = sum(kt_.values())
    alg = 24.0 * n + 16.0 * nd
    line(f"cfg4 per-rank device leg at N={world}, items form (1e9 fact rows + 1/{world} dim per rank)", n, wall, alg, kms,
         "k_slice_partition (per-destination layout) + k_region_pack + k_slice_probe (received regions)", None,
         {"kernel_split_ms": kt_, "items_packed": sent, "items_received": recv,
          "xgmi_bytes_per_rank": 10.0 * (sent - sent // world),
          "note": "frac on SURVEY §8(d)'s 24 B / fact row + 16 B / dim row; the receive side stood in by this "
                  "rank's own block x 8 (uniform keys); RCCL all-to-all time excluded; wall includes the "
                  "stand-in copies"})


def cfg5_leg(ctx, scale, world=8):
    """BASELINE config 5's per-rank device leg at N = 8, on one GPU: what one rank of the distributed
    ROW_NUMBER() OVER (PARTITION BY k ORDER BY v) runs besides the two RCCL all-to-alls
    (DistributedExecutor.row_number -> _moved_window; window.rs:32-226 on each rank):
      1. the 8-way hash exchange pass over the rank's 1.25e8 rows (qeh_partition_hash_move: k, v read
         once, written partition-major);
      2. the local ROW_NUMBER over what the rank receives: partition 0 of every rank's rows (the
         1e9-row table is generated whole and each rank's 1/8 moved, so the received rows are the real
         ones, source-rank-major);
      3. the reverse pass (qeh_partition_hash_unmove): the row numbers that come back, partition-major,
         gathered into the rank's input order.
    Algorithmic bytes: 16 B read + 8 B written per row of the rank."""
    n = int(1e9 * scale)
    nr = n // world
    k = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 7, n, 2 ** 20)
    v = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 8, n, 2 ** 62, lo=-(2 ** 61))
    rk, rv = ctx.slice(k, 0, nr), ctx.slice(v, 0, nr)  # rank 0's rows
    recv_k, recv_v = [], []
    for r in range(world):  # what rank 0 receives: partition 0 of every rank's rows, source-rank-major
        c, m = ctx.partition_hash_move([ctx.slice(k, r * nr, nr)], world, [ctx.slice(k, r * nr, nr), ctx.slice(v, r * nr, nr)])
        recv_k.append(ctx.concat([ctx.slice(m[0], 0, int(c[0]))]))
        recv_v.append(ctx.concat([ctx.slice(m[1], 0, int(c[0]))]))
        for q in m:
            q.release()
    rk_all, rv_all = ctx.concat(recv_k), ctx.concat(recv_v)
    for q in recv_k + recv_v:
        q.release()
    recv = len(rk_all)
    counts0, m0 = ctx.partition_hash_move([rk], world, [rk])
    m0[0].release()
    back = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 9, nr, 2 ** 30)  # stands in for the returned numbers

    def leg1():
        c, m = ctx.partition_hash_move([rk], world, [rk, rv])
        for q in m:
            q.release()
        return c

    def leg2():
        rn = ctx.row_number([rk_all], [rv_all], [True])
        rn.release()

    def leg3():
        out = ctx.partition_hash_unmove(rk, world, [back])
        for q in out:
            q.release()
    names = ["partition_move", "radix_pass", "sort_encode", "row_number", "window_partition", "window_sort",
             "window_place", "w3_partition", "w3_sort", "w3_place"]
    w1, k1, _ = timed(ctx, leg1, 5, names)
    w2, k2, _ = timed(ctx, leg2, 3, names)
    w3, k3, _ = timed(ctx, leg3, 5, names)
    kms2 = sum(v_ for n_, v_ in k2.items() if n_ != "partition_move")
    legs = {"exchange_pass": {"ms": k1["partition_move"], "wall_ms": w1 * 1e3, "hbm_bytes_moved": 32.0 * nr},
            "local_row_number": {"ms": kms2, "wall_ms": w2 * 1e3, "rows": recv, "kernels": {n_: v_ for n_, v_ in k2.items() if v_}},
            "unmove_pass": {"ms": k3["partition_move"], "wall_ms": w3 * 1e3, "hbm_bytes_moved": 17.0 * nr}}
    kms = k1["partition_move"] + kms2 + k3["partition_move"]
    xgmi = (world - 1) / world * (16.0 * nr + 8.0 * recv)
    line(f"cfg5 per-rank device leg at N={world} (ROW_NUMBER, 1e9 rows, 1/{world} per rank)", nr, w1 + w2 + w3,
         24.0 * nr, kms, "k_part_scatter_small (exchange), k_window passes (local ROW_NUMBER), k_part_gather_small (unmove)",
         None, {"legs": legs, "received_rows": recv, "rank0_partition_counts": [int(q) for q in counts0],
                "xgmi_bytes_per_rank": xgmi,
                "note": "frac on SURVEY §8(d)'s 24 B per row of the rank; RCCL all-to-all time excluded (8-GPU runs "
                        "are the driver's); wall = sum of the legs"})


def cfg_filter(ctx, scale):
    n = int(5e8 * scale)
    x = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 1, n, 100)
    k = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 2, n, 1024)
    v = ctx.generate(abi.GEN_UNIT_F64, SEED, 3, n)
    pred = binop(col(0), BinaryOp.Greater, lit(49))

    def fn():
        out, rows = ctx.filter([x, k, v], pred)
        for c in out:
            c.release()
        return rows
    wall, kt, rows = timed(ctx, fn, 5, ["filter"])
    line("filter 5e8 x3 cols", n, wall, 24.0 * n + 24.0 * rows, kt["filter"], "k_filter<1>", None,
         {"selected": rows})


def cfg_limit(ctx, scale):
    """SELECT x, k, v FROM t WHERE x > 49 LIMIT 1000 over 5e8 rows: qeh_filter_limit stops claiming
    tiles once 1000 rows are placed (the reference filters every row, then slices)."""
    n = int(5e8 * scale)
    x = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 1, n, 100)
    k = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 2, n, 1024)
    v = ctx.generate(abi.GEN_UNIT_F64, SEED, 3, n)
    pred = binop(col(0), BinaryOp.Greater, lit(49))

    def fn():
        out, rows = ctx.filter([x, k, v], pred, max_rows=1000)
        for c in out:
            c.release()
        return rows
    wall, kt, rows = timed(ctx, fn, 20, ["filter"])
    line("filter+limit 5e8 x3 cols LIMIT 1000", n, wall, None, kt["filter"], "k_filter_fast (capped)", None,
         {"selected": rows, "note": "rows_per_s counts the table's rows; only the leading tiles are read"})


def cfg_plan(ctx, scale):
    """The metric query through QueryExecutor.execute from host Arrow batches (the reference's
    MemoryDataSource path): cold = every execute imports the Scan batches over PCIe; cached = the
    sources carry a cache key, so the device copy from the first execute is reused."""
    import pyarrow as pa
    from qe_hip import (AggregateExpr, Filter, HashAggregate, HashJoin, JoinType, MemoryDataSource,
                        QueryExecutor, Scan)
    from qe_hip.expr import Column
    n, nd = int(1e8 * scale), int(1e7 * scale)
    cols = {"f.x": (abi.GEN_UNIFORM_MOD, 1, 100), "f.k": (abi.GEN_UNIFORM_MOD, 2, nd), "f.v": (abi.GEN_UNIT_F64, 3, 0)}
    fact = pa.table({name: ctx.generate(kind, SEED, cid, n, mod).to_numpy()[0] for name, (kind, cid, mod) in cols.items()})
    dim = pa.table({"d.k": ctx.generate(abi.GEN_PERMUTATION, SEED, 0, nd, nd).to_numpy()[0],
                    "d.g": ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 5, nd, 1024).to_numpy()[0]})
    qx = QueryExecutor(ctx)
    out = {}
    for mode in ("cold", "cached"):
        cache = mode == "cached"
        fs = MemoryDataSource(fact.schema, fact.to_batches(max_chunksize=1 << 23), device_cache=cache)
        ds = MemoryDataSource(dim.schema, dim.to_batches(), device_cache=cache)
        join = HashJoin(Scan(fs), Scan(ds), JoinType.Inner, binop(Column("f.k", 1), BinaryOp.Equal, Column("d.k", 3)))
        plan = HashAggregate(Filter(join, binop(Column("f.x", 0), BinaryOp.Greater, lit(49))), [Column("d.g", 4)],
                             [AggregateExpr(AF.Sum, Column("f.v", 2)), AggregateExpr(AF.Count, Column("f.v", 2))])
        qx.execute(plan)
        reps = 3 if mode == "cold" else 10
        t0 = time.perf_counter()
        for _ in range(reps):
            res = qx.execute(plan)
        wall = (time.perf_counter() - t0) / reps
        out[mode] = wall
        line(f"plan metric query 1e8 x 1e7 from host Arrow ({mode})", n, wall, None, None, None, None,
             {"groups": res[0].num_rows, "host_bytes_per_execute": 24 * n + 16 * nd if mode == "cold" else 0,
              "pcie_inclusive_GBs": (24 * n + 16 * nd) / wall / 1e9 if mode == "cold" else None})
        qx.cache_evict()


UTF8_DICT_KERNELS = ["utf8_dict_insert", "utf8_dict_compact", "utf8_dict_order", "utf8_dict_codes", "radix_pass",
                     "sort_encode", "scan"]


def upload_utf8_raw(ctx, offs, data):
    """A non-null Utf8 device column from host int32 offsets and uint8 bytes (no Python strings)."""
    from qe_hip.device import DeviceColumn
    po, pd = ctx.alloc(offs.nbytes), ctx.alloc(max(data.nbytes, 8))
    ctx.h2d(po, offs)
    ctx.h2d(pd, data)
    c = abi.QehColumn(dtype=abi.DT_UTF8, owned=0, length=len(offs) - 1, offset=0, null_count=0, values=pd, offsets=po,
                      values_bytes=int(offs[-1]))
    return DeviceColumn(ctx, c, [po, pd])


def utf8_key_report(ctx, cfg, n, key, string_bytes, op_utf8, op_codes, op_kernels, reps=5):
    """One line: the query over the Utf8 key, the same query over its pre-encoded Int32 codes (the
    existing integer path, same process), the encode step alone and its share, and the encode
    pass against its floor (offsets read + string bytes read + codes written, at 8 TB/s)."""
    def enc():
        c, d = ctx.utf8_dict_encode(key)
        c.release()
        d.release()
    enc_wall, enc_kt, _ = timed(ctx, enc, reps, UTF8_DICT_KERNELS)
    codes, dic = ctx.utf8_dict_encode(key)
    wall_u, kt_u, _ = timed(ctx, lambda: op_utf8(key), reps, list(dict.fromkeys(UTF8_DICT_KERNELS + op_kernels)))
    wall_c, kt_c, _ = timed(ctx, lambda: op_codes(codes), reps, op_kernels)
    alg = 4.0 * (n + 1) + string_bytes + 4.0 * n
    floor_ms = alg / (PEAK * 1e9) * 1e3
    enc_kernel_ms = sum(enc_kt.values())
    line(cfg, n, wall_u, alg, enc_kernel_ms, "k_dict_insert (+ compact, order, codes)", None,
         {"distinct": len(dic), "utf8_key_wall_ms": wall_u * 1e3, "utf8_key_kernel_ms": sum(kt_u.values()),
          "int32_codes_wall_ms": wall_c * 1e3, "int32_codes_kernel_ms": sum(kt_c.values()),
          "encode_wall_ms": enc_wall * 1e3, "encode_kernel_ms": enc_kernel_ms,
          "encode_kernels_ms": enc_kt, "encode_share_of_wall": enc_wall / wall_u,
          "encode_floor_ms": floor_ms, "encode_frac_of_floor": floor_ms / enc_kernel_ms if enc_kernel_ms else None,
          "encode_wall_frac_of_floor": floor_ms / (enc_wall * 1e3)})


def cfg_utf8_groupby(ctx, scale):
    """SELECT s, COUNT(v), SUM(v) FROM t GROUP BY s: 1e8 rows over 1024 distinct strings of 8-24 bytes."""
    n, nd = int(1e8 * scale), 1024
    r = np.random.default_rng(SEED)
    pool = [bytes(r.integers(97, 123, int(l), dtype=np.uint8)) + b"%04d" % i for i, l in enumerate(r.integers(4, 21, nd))]
    small = ctx.upload(pool)
    k = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 2, n, nd)
    key = ctx.take(small, k)  # the 1e8-row Utf8 column, gathered on the device
    v = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 4, n, 2 ** 21, lo=-(2 ** 20))
    aggs = [(AF.Count, 0), (AF.Sum, 0)]
    utf8_key_report(ctx, "utf8 group-by 1e8 rows, 1024 strings of 8-24 B", n, key, float(key.c.values_bytes),
                    lambda kc: ctx.hash_aggregate([kc], [v], aggs), lambda kc: ctx.hash_aggregate([kc], [v], aggs),
                    ["aggregate_rows", "group_insert", "gather"])


def cfg_utf8_sort(ctx, scale):
    """SELECT ... ORDER BY s: 1e8 rows of all-distinct 16-byte strings."""
    n = int(1e8 * scale)
    hexd = np.frombuffer(b"0123456789abcdef", np.uint8)
    data = np.empty(n * 16, np.uint8)
    shifts = np.arange(60, -4, -4, dtype=np.uint64)
    step = 5_000_000
    for a in range(0, n, step):  # 16 hex digits of a bijection of the row number
        x = np.arange(a, min(a + step, n), dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(SEED)
        data[a * 16:(a + len(x)) * 16] = hexd[((x[:, None] >> shifts) & np.uint64(15)).astype(np.intp)].ravel()
    offs = (np.arange(n + 1, dtype=np.int64) * 16).astype(np.int32)
    key = upload_utf8_raw(ctx, offs, data)
    del data
    utf8_key_report(ctx, "utf8 order-by 1e8 rows, all-distinct 16 B strings", n, key, 16.0 * n,
                    lambda kc: ctx.sort_indices([kc], [True]), lambda kc: ctx.sort_indices([kc], [True]),
                    ["radix_pass", "sort_encode"], reps=3)


def cfg_utf8_join(ctx, scale):
    """SELECT ... FROM probe JOIN build ON probe.s = build.s: 1e8 probe rows against 1e6 distinct build
    strings of 8-24 bytes, about 10 % of the probe rows absent from the build side."""
    n, nb = int(1e8 * scale), max(int(1e6 * scale), 16)
    npool = nb + nb // 9  # the probe draws from the build strings and 1/9 as many others: 10 % absent
    r = np.random.default_rng(SEED)
    lens = r.integers(8, 25, npool).astype(np.int64)
    offs = np.zeros(npool + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    data = r.integers(97, 123, int(offs[-1]), dtype=np.uint8)
    hexd = np.frombuffer(b"0123456789abcdef", np.uint8)
    ids = np.arange(npool, dtype=np.uint64)[:, None] >> np.arange(28, -4, -4, dtype=np.uint64)
    data[(offs[:-1, None] + np.arange(8)).ravel()] = hexd[(ids & np.uint64(15)).astype(np.intp)].ravel()  # distinct
    offs32 = offs.astype(np.int32)
    pool = upload_utf8_raw(ctx, offs32, data)
    build = upload_utf8_raw(ctx, offs32[:nb + 1], data[:offs[nb]])
    probe = ctx.take(pool, ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 2, n, npool))  # gathered on the device
    pv = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 4, n, 2 ** 21, lo=-(2 ** 20))
    bv = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 5, nb, 2 ** 21, lo=-(2 ** 20))
    enc_names = ["utf8_dict_insert", "utf8_dict_lookup", "utf8_dict_compact", "utf8_dict_codes", "scan"]

    def enc():
        b, p, _ = ctx.utf8_join_encode(build, probe)
        b.release()
        p.release()
    enc_wall, enc_kt, _ = timed(ctx, enc, 5, enc_names)
    bc, pc, d = ctx.utf8_join_encode(build, probe)
    join_names = ["join_build", "join_count", "join_probe", "join_gather", "join_mat"]

    def joined(res):
        for c in res[0] + res[1]:
            c.release()
        return res[2]
    wall_u, kt_u, rows = timed(ctx, lambda: joined(ctx.hash_join(0, probe, [pv], build, [bv])), 5, enc_names + join_names)
    wall_c, kt_c, _ = timed(ctx, lambda: joined(ctx.hash_join_inner(pc, [pv], bc, [bv])), 5, join_names)

    def dict_enc():  # k_dict_insert over the probe column itself: the per-row yardstick of the lookup
        c, dic = ctx.utf8_dict_encode(probe)
        c.release()
        dic.release()
    _, ins_kt, _ = timed(ctx, dict_enc, 2, ["utf8_dict_insert"])
    probe_bytes = float(probe.c.values_bytes)
    alg = 4.0 * (n + 1) + probe_bytes + 4.0 * n + n / 8.0  # probe offsets + bytes read, codes + validity written
    floor_ms = alg / (PEAK * 1e9) * 1e3
    lookup_ms = enc_kt["utf8_dict_lookup"]
    line("utf8 join 1e8 probe rows, 1e6 build strings of 8-24 B, 10 % absent", n, wall_u, alg, lookup_ms, "k_dict_lookup", None,
         {"build_rows": nb, "distinct": d, "joined_rows": rows, "probe_string_bytes": probe_bytes,
          "encode_wall_ms": enc_wall * 1e3, "encode_kernel_ms": sum(enc_kt.values()), "encode_kernels_ms": enc_kt,
          "lookup_floor_ms": floor_ms, "lookup_frac_of_floor": floor_ms / lookup_ms if lookup_ms else None,
          "lookup_ns_per_row": lookup_ms * 1e6 / n, "insert_ns_per_build_row": enc_kt["utf8_dict_insert"] * 1e6 / nb,
          "insert_over_probe_column_ms": ins_kt["utf8_dict_insert"],
          "insert_over_probe_column_ns_per_row": ins_kt["utf8_dict_insert"] * 1e6 / n,
          "utf8_join_wall_ms": wall_u * 1e3, "utf8_join_kernels_ms": kt_u,
          "int32_codes_join_wall_ms": wall_c * 1e3, "int32_codes_join_kernels_ms": kt_c,
          "encode_share_of_join_wall": enc_wall / wall_u})


TOPK_KERNELS = ["topk_select", "radix_pass", "sort_encode", "gather", "scan"]


def topk_ab(ctx, key, limit, reps, select_env):
    """qeh_sort_indices_limit with the select path (`select_env` set) and with the full sort
    (QEH_NO_TOPK=1), interleaved in this process: per side the median wall ms and the kernel ms per
    call by timer name."""
    sides = {"select": select_env, "full": {"QEH_NO_TOPK": "1"}}
    knobs = ["QEH_NO_TOPK", "QEH_TOPK_FORCE", "QEH_TOPK_MIN_ROWS"]
    wall = {s: [] for s in sides}
    kms = {s: dict.fromkeys(TOPK_KERNELS, 0.0) for s in sides}
    ctx.timing(True)
    for rep in range(reps + 1):  # rep 0 warms both sides up
        for side, env in sides.items():
            for kn in knobs:
                os.environ.pop(kn, None)
            os.environ.update(env)
            ctx.timing_reset()
            ctx.sync()
            t0 = time.perf_counter()
            ctx.sort_indices_limit([key], [True], limit).release()
            ctx.sync()
            dt = time.perf_counter() - t0
            if rep:
                wall[side].append(dt * 1e3)
                for kn in TOPK_KERNELS:
                    kms[side][kn] += ctx.kernel_time(kn)[0] / reps
    ctx.timing(False)
    for kn in knobs:
        os.environ.pop(kn, None)
    return {s: float(np.median(wall[s])) for s in sides}, kms


def cfg_topk(ctx, scale):
    """SELECT ... ORDER BY k LIMIT 100 over 1e8 rows: qeh_sort_indices_limit's select path against
    the full sort cut to 100 rows (QEH_NO_TOPK=1), same process, interleaved; then the sweeps the
    three fallback constants of csrc/k_topk.hip are read from (QEH_TOPK_FORCE=1: the select path at
    any limit, row count and candidate share)."""
    n = int(1e8 * scale)
    keys = {"int64 spread over 2^62": lambda m: ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 2, m, 2 ** 62, lo=-(2 ** 61)),
            "float64 in [0, 1)": lambda m: ctx.generate(abi.GEN_UNIT_F64, SEED, 3, m),
            "int64 in [0, 1024) (heavy ties)": lambda m: ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 4, m, 1024)}
    for name, gen in keys.items():
        key = gen(n)
        wall, kms = topk_ab(ctx, key, 100, 5, {})
        sel_ms = kms["select"]["topk_select"]
        taken = sel_ms > 0 and kms["select"]["radix_pass"] < 0.5 * kms["full"]["radix_pass"]
        line(f"topk ORDER BY k LIMIT 100, {n} rows, {name}", n, wall["select"] * 1e-3, None, sel_ms, "k_topk_hist", None,
             {"select_wall_ms": wall["select"], "full_sort_wall_ms": wall["full"],
              "speedup_wall": wall["full"] / wall["select"], "select_path_taken": bool(taken),
              "select_kernels_ms": kms["select"], "full_sort_kernels_ms": kms["full"],
              "read_floor_ms_per_pass": 8.0 * n / (PEAK * 1e9) * 1e3,
              "note": "floor = passes x n x 8 B of key reads; passes = range + select digits + count + write"})
        del key
    force = {"QEH_TOPK_FORCE": "1"}
    for m in [int(x * scale) for x in (1e4, 1e5, 1e6, 2e6, 4e6, 1e7, 1e8)]:  # limit / n and n
        key = keys["int64 spread over 2^62"](m)
        for share in (1e-6, 1e-5, 1e-4, 1e-3, 1e-2, 1 / 32, 1 / 16, 1 / 8, 1 / 4, 1 / 2):
            limit = max(1, int(m * share))
            wall, _ = topk_ab(ctx, key, limit, 3, force)
            print(json.dumps({"config": "topk sweep limit/n", "rows": m, "limit": limit, "limit_share": share,
                              "select_wall_ms": wall["select"], "full_sort_wall_ms": wall["full"],
                              "speedup_wall": wall["full"] / wall["select"]}), flush=True)
        del key
    for m in [int(x * scale) for x in (1e6, 1e8)]:  # candidate share: keys in [0, R), about m / R rows tie at the threshold
        for r in (2, 4, 8, 16, 32, 64, 128, 256, 512):
            key = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 5, m, r)
            wall, _ = topk_ab(ctx, key, 100, 3, force)
            print(json.dumps({"config": "topk sweep candidate share", "rows": m, "limit": 100, "cand_share": 1.0 / r,
                              "select_wall_ms": wall["select"], "full_sort_wall_ms": wall["full"],
                              "speedup_wall": wall["full"] / wall["select"]}), flush=True)
            del key


def cfg_semi(ctx, scale):
    """k IN (set) as a nullable BOOL column (qeh_in_set, csrc/k_semi.hip), both set forms.  Every probe key
    lies inside the set's range, so every row pays its lookup (none is answered by the range check)."""
    nd = 10_000_000
    shapes = [("bitmap", int(1e9 * scale),
               lambda n: ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 2, n, nd),
               lambda: ctx.generate(abi.GEN_PERMUTATION, SEED, 0, nd, nd), "dense set: a permutation of [0, 1e7)"),
              ("hash", int(1e8 * scale),
               lambda n: ctx.generate(abi.GEN_SPARSE_KEY, SEED, 2, n, nd),
               lambda: ctx.generate(abi.GEN_SPARSE_KEY, SEED, 2, nd, 0), "sparse set: 1e7 distinct 64-bit keys")]
    for form, n, gen_probe, gen_set, what in shapes:
        probe, sset = gen_probe(n), gen_set()

        def semi():
            out = ctx.in_set(probe, sset)
            out.release()
        wall, kt, _ = timed(ctx, semi, 5, ["semi_probe_bitmap", "semi_probe_hash", "semi_build_bitmap", "semi_build_hash"])
        taken = "bitmap" if kt["semi_probe_bitmap"] > 0 else "hash"

        def join():  # what the parent could do: the pairs of an inner join, probe key only (the set is distinct)
            p, b, rows = ctx.hash_join_inner(probe, [probe], sset, [])
            for c in p + b:
                c.release()
            return rows
        jwall, jkt, jrows = timed(ctx, join, 3, ["join_probe", "join_gather", "join_build"])
        probe_ms = kt["semi_probe_" + taken]
        alg = (8.0 + 1.0 / 8.0) * n
        line(f"semi k IN (set), {n} probes x {nd} keys, {form} form", n, wall, alg, probe_ms, "k_semi_probe", None,
             {"set": what, "form_taken": taken, "build_ms": kt["semi_build_" + taken],
              "byte_floor_ms": alg / (PEAK * 1e9) * 1e3, "probe_over_floor": probe_ms / (alg / (PEAK * 1e9) * 1e3),
              "hash_join_inner_probe_key_only_ms": jwall * 1e3, "hash_join_inner_kernels_ms": jkt,
              "hash_join_inner_rows": jrows, "speedup_vs_hash_join_inner_wall": jwall / wall})
        del probe, sset


TS_KERNELS = ["ts_match_stream", "ts_match_rows"]


def ts_documents(n, block=100_000):
    """n documents of about 64 bytes as (int32 offsets, uint8 bytes): 7 to 11 words of a 32-word
    vocabulary in mixed case, joined by mixed separators.  One block of `block` documents is drawn
    and repeated (each repeat lies at its own addresses, so nothing is re-read from a cache)."""
    rng = np.random.default_rng(SEED)
    vocab = ["gpu", "kernel", "wave", "lds", "cache", "vector", "scalar", "memory", "stream", "query", "index", "token",
             "match", "text", "search", "engine", "column", "batch", "filter", "join", "hash", "sort", "plan", "node",
             "GPU", "Kernel", "Wave64", "LDS", "Query", "hbm3e", "x86", "mi355x"]
    seps = [" ", " ", " ", ", ", "\t", ". ", "_", "-", "\n", "  "]
    docs = []
    for _ in range(min(block, n)):
        k = int(rng.integers(7, 12))
        w = rng.integers(0, len(vocab), k)
        s = rng.integers(0, len(seps), k)
        docs.append("".join(vocab[a] + seps[b] for a, b in zip(w, s)).encode())
    lens = np.array([len(d) for d in docs], np.int64)
    reps = -(-n // len(docs))
    data = np.tile(np.frombuffer(b"".join(docs), np.uint8), reps)
    offs = np.zeros(reps * len(docs) + 1, np.int64)
    offs[1:] = np.cumsum(np.tile(lens, reps))
    assert offs[n] < 2 ** 31
    return offs[:n + 1].astype(np.int32), data[:offs[n]], docs


def cfg_tsmatch(ctx, scale):
    """to_tsvector(doc) @@ to_tsquery('gpu & kernel') over 1e7 documents through qeh_eval: the stream
    kernel (k_ts_match_stream) against the row-per-lane kernel (QEH_NO_TS_STREAM=1), interleaved in
    this process, one warm-up and 5 timed calls each, medians of wall and of kernel time; GB/s over the bytes read (values + offsets;
    the column has no validity)."""
    from qe_hip import ScalarFunction, ScalarFunctionType as F
    n = int(1e7 * scale)
    offs, data, docs = ts_documents(n)
    doc = upload_utf8_raw(ctx, offs, data)
    expr = binop(ScalarFunction(F.ToTsVector, [col(0)]), BinaryOp.TsMatch, ScalarFunction(F.ToTsQuery, [lit("gpu & kernel")]))
    sides = {"stream": {}, "rows": {"QEH_NO_TS_STREAM": "1"}}
    wall = {s: [] for s in sides}
    kms = {s: {k: [] for k in TS_KERNELS} for s in sides}  # per timed call
    selected = {}
    ctx.timing(True)
    for rep in range(6):  # rep 0 warms both sides up
        for side, env in sides.items():
            os.environ.pop("QEH_NO_TS_STREAM", None)
            os.environ.update(env)
            ctx.timing_reset()
            ctx.sync()
            t0 = time.perf_counter()
            out = ctx.eval([doc], expr)
            ctx.sync()
            dt = time.perf_counter() - t0
            if rep:
                wall[side].append(dt * 1e3)
                for kn in TS_KERNELS:
                    kms[side][kn].append(ctx.kernel_time(kn)[0])
            else:
                selected[side] = int(out.to_numpy()[0].sum())
            out.release()
    ctx.timing(False)
    os.environ.pop("QEH_NO_TS_STREAM", None)
    alg = float(data.nbytes + offs.nbytes)
    sample = sum(1 for d in docs if {b"gpu", b"kernel"} <= set(re.findall(rb"[0-9a-z]+", d.lower())))
    res = {}
    for side, kern in (("stream", "ts_match_stream"), ("rows", "ts_match_rows")):
        med = {k: float(np.median(v)) for k, v in kms[side].items()}
        ms = med[kern]
        res[side] = {"wall_ms_median": float(np.median(wall[side])), "kernel_ms_median": ms, "kernels_ms_median": med,
                     "GBs": alg / (ms * 1e-3) / 1e9 if ms else None, "rows_true": selected[side]}
    line(f"tsmatch to_tsvector(doc) @@ to_tsquery('gpu & kernel'), {n} rows, {data.nbytes / n:.1f} B/doc", n,
         res["stream"]["wall_ms_median"] * 1e-3, alg, res["stream"]["kernel_ms_median"], "k_ts_match_stream", None,
         {"stream": res["stream"], "rows_kernel": res["rows"], "byte_floor_ms": alg / (PEAK * 1e9) * 1e3,
          "kernel_speedup_stream_over_rows": res["rows"]["kernel_ms_median"] / res["stream"]["kernel_ms_median"]
          if res["stream"]["kernel_ms_median"] else None,
          "true_share_of_first_block_on_host": sample / len(docs), "both_kernels_agree": selected["stream"] == selected["rows"]})


def cfg_temporal(ctx, scale):
    """pgwire DataRow text of 1e7 rows x (Int64, Date32, Timestamp(us)) against the same call over three
    Int64 columns (the path these columns' values took before they had a type), interleaved in this
    process: one warm-up and 5 timed calls each, medians, kernel times by name, and the ratio per
    output byte.  The dates cover years 1900-2100, half the timestamps carry a microsecond fraction."""
    n = int(1e7 * scale)
    r = np.random.default_rng(SEED)
    k = ctx.generate(abi.GEN_UNIFORM_MOD, SEED, 2, n, 1 << 40)
    days = r.integers(-25567, 47482, n).astype(np.int32)
    us = r.integers(-25567 * 86400, 47482 * 86400, n) * 10 ** 6 + np.where(r.random(n) < 0.5, 0, r.integers(0, 10 ** 6, n))
    d32, tsu = ctx.upload(days, dtype=abi.DT_DATE32), ctx.upload(us, dtype=abi.DT_TIMESTAMP_US)
    sides = {"temporal": [k, d32, tsu], "int64": [k, ctx.upload(days.astype(np.int64)), ctx.upload(us)]}
    kernels = ["encode_len", "encode_write"]
    wall = {s: [] for s in sides}
    kms = {s: {kn: [] for kn in kernels} for s in sides}
    nbytes = {}
    ctx.timing(True)
    for it in range(6):  # the first round warms both sides up
        for side, cols in sides.items():
            ctx.timing_reset()
            ctx.sync()
            t0 = time.perf_counter()
            out = ctx.encode_pg_datarows(cols)
            ctx.sync()
            dt = time.perf_counter() - t0
            nbytes[side] = out.c.values_bytes
            out.release()
            if it:
                wall[side].append(dt * 1e3)
                for kn in kernels:
                    kms[side][kn].append(ctx.kernel_time(kn)[0])
    ctx.timing(False)
    res = {}
    for side in sides:
        med = {kn: float(np.median(v)) for kn, v in kms[side].items()}
        res[side] = {"wall_ms_median": float(np.median(wall[side])), "kernels_ms_median": med,
                     "kernel_ms": sum(med.values()), "encoded_bytes": nbytes[side],
                     "kernel_ns_per_output_byte": sum(med.values()) * 1e6 / nbytes[side]}
    t, i = res["temporal"], res["int64"]
    in_bytes = 20.0 * n
    line(f"pgwire DataRow text encoding {n} x (Int64, Date32, Timestamp(us)) vs 3 x Int64", n, t["wall_ms_median"] * 1e-3,
         in_bytes + t["encoded_bytes"], t["kernel_ms"], "k_pg_row_len + k_pg_row_write (civil date from days)", None,
         {"temporal": t, "int64": i, "kernel_ratio_temporal_over_int64": t["kernel_ms"] / i["kernel_ms"],
          "per_output_byte_ratio": t["kernel_ns_per_output_byte"] / i["kernel_ns_per_output_byte"]})


CSV_KERNELS = ["csv_chunks", "csv_pick", "csv_starts", "csv_fields", "csv_utf8", "scan"]


def cfg_csv(ctx, scale):
    """CsvDataSource::scan / load_csv on the device.  The file is generated once on the host; five timed
    runs after a warm-up per arm, all in this process."""
    import pyarrow as pa
    import pyarrow.csv as pacsv
    n = int(1e7 * scale)
    rng = np.random.default_rng(SEED)
    ints = rng.integers(-2**40, 2**40, n).tolist()
    floats = (rng.standard_normal(n) * 1e3).tolist()
    words = ["".join(chr(97 + int(c)) for c in rng.integers(0, 26, int(k))) for k in rng.integers(4, 13, 4096)]
    widx = rng.integers(0, len(words), n).tolist()
    dates = np.datetime_as_string(np.datetime64("1970-01-01") + rng.integers(0, 20000, n)).tolist()
    parts = ["k,v,s,d\n"]
    step = 1_000_000
    for lo in range(0, n, step):
        parts.append("".join(f"{a},{b!r},{words[w]},{d}\n" for a, b, w, d in
                             zip(ints[lo:lo + step], floats[lo:lo + step], widx[lo:lo + step], dates[lo:lo + step])))
    data = "".join(parts).encode()
    del parts, ints, floats, widx, dates
    schema = pa.schema([("k", pa.int64()), ("v", pa.float64()), ("s", pa.string()), ("d", pa.date32())])
    dev = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    torch.cuda.synchronize()
    sizes = {}

    def run(src):
        cols = ctx.scan_csv(src, schema)
        sizes["utf8"] = cols[2].c.values_bytes
        sizes["rows"] = len(cols[0])
        for c in cols:
            c.release()

    arms = {}
    for arm, src in (("device_bytes", dev), ("host_bytes", data)):
        walls = []
        run(src)
        ctx.sync()
        ctx.timing(True)
        ctx.timing_reset()
        for _ in range(5):
            t0 = time.perf_counter()
            run(src)
            ctx.sync()
            walls.append(time.perf_counter() - t0)
        kt = {k: ctx.kernel_time(k)[0] / 5 for k in CSV_KERNELS}
        patch_ms, patched = ctx.kernel_time("csv_float_patch")
        ctx.timing(False)
        arms[arm] = {"wall_ms": [w * 1e3 for w in walls], "wall_ms_median": sorted(walls)[2] * 1e3, "kernel_ms": sum(kt.values()),
                     "kernel_split_ms": kt, "float_cells_parsed_on_host_share": patched / 5 / max(n, 1),
                     "float_patch_host_ms": patch_ms / 5}
    assert sizes["rows"] == n
    pa.set_cpu_count(16)
    opts = dict(convert_options=pacsv.ConvertOptions(column_types=schema))
    pacsv.read_csv(pa.BufferReader(data), **opts)
    host = []
    for _ in range(5):
        t0 = time.perf_counter()
        pacsv.read_csv(pa.BufferReader(data), **opts)
        host.append(time.perf_counter() - t0)
    size = len(data)
    written = n * (8 + 8 + 4 + 4) + sizes["utf8"]
    floor_bytes = 4 * size + written  # k_csv_chunks, k_csv_starts, k_csv_fields, k_csv_utf8 each read the file
    d = arms["device_bytes"]
    dominant = max((k for k in CSV_KERNELS), key=lambda k: d["kernel_split_ms"][k])
    cpu = {"value": n / sorted(host)[2], "unit": "rows/s", "cores": 16, "kind": "pyarrow.csv.read_csv, pa.set_cpu_count(16)",
           "ms": [h * 1e3 for h in host], "GBs": size / sorted(host)[2] / 1e9}
    line("qeh_scan_csv 1e7 x (Int64, Float64 shortest repr, Utf8 4-12 B, Date32), bytes on the device", n,
         d["wall_ms_median"] * 1e-3, float(floor_bytes), d["kernel_ms"], dominant, cpu,
         {"file_bytes": size, "file_GBs_wall": size / (d["wall_ms_median"] * 1e-3) / 1e9, "floor_ms_at_8TBs": floor_bytes / 8e12 * 1e3,
          "kernel_over_floor": d["kernel_ms"] / (floor_bytes / 8e12 * 1e3), "device_bytes": d, "host_bytes": arms["host_bytes"],
          "speedup_vs_pyarrow16_device_bytes": sorted(host)[2] * 1e3 / d["wall_ms_median"],
          "speedup_vs_pyarrow16_with_upload": sorted(host)[2] * 1e3 / arms["host_bytes"]["wall_ms_median"]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="cfg2,cfg3,cfg5,filter")
    ap.add_argument("--scale", type=float, default=1.0)
    args = ap.parse_args()
    torch.cuda.set_device(0)
    s = torch.cuda.Stream()
    torch.cuda.set_stream(s)
    ctx = qe_hip.Context(0)
    ctx.set_stream(s.cuda_stream)
    for name in args.only.split(","):
        {"cfg2": cfg2, "cfg3": cfg3, "cfg5": cfg5, "filter": cfg_filter, "limit": cfg_limit,
         "plan": cfg_plan, "left": lambda c, s: cfg_outer(c, s, 1), "full": lambda c, s: cfg_outer(c, s, 3),
         "merge": cfg_merge, "encode": cfg_encode, "shapes": cfg_metric_shapes, "partition": cfg_partition, "cfg3w": cfg3_wide, "window": cfg_window,
         "cfg4leg": cfg4_leg, "cfg4items": cfg4_items_leg, "cfg5leg": cfg5_leg,
         "window_lsd": cfg_window_lsd, "utf8_groupby": cfg_utf8_groupby, "utf8_sort": cfg_utf8_sort, "utf8_join": cfg_utf8_join,
         "topk": cfg_topk, "semi": cfg_semi, "tsmatch": cfg_tsmatch, "temporal": cfg_temporal, "csv": cfg_csv}[name](ctx, args.scale)
        ctx.sync()
        abi.check(ctx.lib.qeh_pool_trim(ctx.h))
    ctx.close()


if __name__ == "__main__":
    main()
