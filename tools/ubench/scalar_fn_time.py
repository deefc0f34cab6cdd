"""String scalar functions against a device-to-device copy of the same bytes (DESIGN.md §5 "Scalar functions").

UPPER over 1e7 rows x 16 B on both of its paths -- str_case_stream (no NULLs) and str_rows (one NULL
row sends the column there) -- and CONCAT of two such columns, each as the sum of its kernels' device
time (HIP events, qeh_kernel_time) and as host time around the whole qeh_eval call, next to a
hipMemcpy device-to-device of the column's bytes in the same run: the floor for anything that reads
and writes them once.  Prints one JSON line.

    python tools/ubench/scalar_fn_time.py [rows] [bytes_per_row]
"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "query-engine_amd"))
import torch  # noqa: F401,E402
import qe_hip  # noqa: E402
from qe_hip import ScalarFunction, ScalarFunctionType as F, abi, col  # noqa: E402
from qe_hip.device import DeviceColumn, pack_bits  # noqa: E402

WARMUP, REPS = 2, 10
KERNELS = ["str_case_stream", "str_rebase_offsets", "str_row_len", "scan", "str_rows"]


def string_column(ctx, n, width, seed, one_null):
    rng = np.random.default_rng(seed)
    data = rng.integers(ord("a"), ord("z") + 1, n * width).astype(np.uint8)
    offs = (np.arange(n + 1, dtype=np.int64) * width).astype(np.int32)
    po, pd = ctx.alloc(offs.nbytes), ctx.alloc(data.nbytes)
    ctx.h2d(po, offs)
    ctx.h2d(pd, data)
    c = abi.QehColumn(dtype=abi.DT_UTF8, owned=0, length=n, offset=0, null_count=0, values=pd, offsets=po,
                      values_bytes=data.nbytes)
    bufs = [po, pd]
    if one_null:
        valid = np.ones(n, bool)
        valid[n // 2] = False
        vb = pack_bits(valid)
        q = ctx.alloc(vb.nbytes)
        ctx.h2d(q, vb)
        c.validity, c.null_count = q, 1
        bufs.append(q)
    return DeviceColumn(ctx, c, bufs)


def timed(ctx, cols, expr):
    """(median host ms per call, device ms per call summed over the kernels, kernels that ran)"""
    host = []
    for rep in range(WARMUP + REPS):
        if rep == WARMUP:
            ctx.timing(True)
            ctx.timing_reset()
        ctx.sync()
        t0 = time.perf_counter()
        out = ctx.eval(cols, expr)
        ctx.sync()
        host.append(1e3 * (time.perf_counter() - t0))
        out.release()
    per = {k: ctx.kernel_time(k) for k in KERNELS}
    ctx.timing(False)
    dev = sum(ms for ms, _ in per.values()) / REPS
    return float(np.median(host[WARMUP:])), dev, {k: round(ms / REPS, 4) for k, (ms, cnt) in per.items() if cnt}


def main():
    n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 10_000_000
    width = int(sys.argv[2]) if len(sys.argv) > 2 else 16
    ctx = qe_hip.Context(0)
    a = string_column(ctx, n, width, 1, False)
    b = string_column(ctx, n, width, 2, False)
    a_null = string_column(ctx, n, width, 1, True)
    nbytes = n * width
    # the floor: the column's bytes copied device to device, many copies per synchronise
    dst = ctx.alloc(nbytes)
    copies = 20
    floor = []
    for rep in range(WARMUP + REPS):
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(copies):
            ctx.copy_d2d(dst, a.c.values, nbytes)
        ctx.sync()
        floor.append(1e3 * (time.perf_counter() - t0) / copies)
    copy_ms = float(np.median(floor[WARMUP:]))
    res = {"rows": n, "bytes_per_row": width, "copy_d2d_ms": round(copy_ms, 4)}
    for name, cols, expr in [("upper_stream", [a], ScalarFunction(F.Upper, [col(0)])),
                             ("upper_rows", [a_null], ScalarFunction(F.Upper, [col(0)])),
                             ("concat2_rows", [a, b], ScalarFunction(F.Concat, [col(0), col(1)]))]:
        host_ms, dev_ms, per = timed(ctx, cols, expr)
        res[name] = {"host_ms": round(host_ms, 4), "device_ms": round(dev_ms, 4), "kernels_ms": per,
                     "device_over_copy": round(dev_ms / copy_ms, 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
