"""The id pass of qeh_range_partition_utf8 against the dictionary route (utf8_dict_encode + range_partition
over the codes): 1e7 rows of 8..24-byte ASCII strings, 7 splitters, alternating, five runs each.
    python tools/probes/range_partition_utf8_ab.py [OUT.jsonl]"""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "query-engine_amd"))
import qe_hip  # noqa: E402
from qe_hip import abi  # noqa: E402
from qe_hip.device import DeviceColumn  # noqa: E402

N = 10_000_000
r = np.random.default_rng(1)
lens = r.integers(8, 25, N).astype(np.int64)
offs = np.zeros(N + 1, np.int32)
offs[1:] = np.cumsum(lens)
data = r.integers(97, 123, int(offs[-1]), dtype=np.uint8)
ctx = qe_hip.Context(0)
po, pd = ctx.alloc(offs.nbytes), ctx.alloc(data.nbytes + 8)
ctx.h2d(po, offs)
ctx.h2d(pd, data)
col = DeviceColumn(ctx, abi.QehColumn(dtype=abi.DT_UTF8, owned=0, length=N, offset=0, null_count=0, values=pd, offsets=po,
                                      values_bytes=int(offs[-1])), [po, pd])
pick = np.sort(r.integers(0, N, 7))
raw = data.tobytes()
splitters = sorted(raw[offs[i]:offs[i + 1]] for i in pick)
ctx.timing(True)
lines = []


def direct():
    ctx.timing_reset()
    t0 = time.perf_counter()
    counts, perm = ctx.range_partition_utf8(col, splitters, True)
    wall = (time.perf_counter() - t0) * 1e3
    ms, launches = ctx.kernel_time("range_partition_utf8")
    return {"route": "range_partition_utf8", "call_ms": round(wall, 3), "id_pass_kernel_ms": round(ms, 3),
            "id_pass_launches": launches, "counts": counts.tolist()}


def dictionary():
    ctx.timing_reset()
    t0 = time.perf_counter()
    codes, dic = ctx.utf8_dict_encode(col)
    t1 = time.perf_counter()
    sp = np.sort(codes.to_numpy()[0][pick].astype(np.int64))  # the splitter rows' codes
    t2 = time.perf_counter()
    counts, perm = ctx.range_partition(codes, sp, True)
    t3 = time.perf_counter()
    ms, _ = ctx.kernel_time("range_partition")
    return {"route": "utf8_dict_encode + range_partition", "call_ms": round((t1 - t0 + t3 - t2) * 1e3, 3),
            "encode_ms": round((t1 - t0) * 1e3, 3), "range_partition_ms": round((t3 - t2) * 1e3, 3),
            "id_pass_kernel_ms": round(ms, 3), "splitter_lookup_on_host_ms_not_counted": round((t2 - t1) * 1e3, 3),
            "counts": counts.tolist()}


direct(), dictionary()  # warm-up: pool allocations, code objects
for i in range(5):
    for fn in (direct, dictionary):
        rec = fn()
        rec["run"] = i
        lines.append(rec)
        print(json.dumps(rec), flush=True)
a = [x for x in lines if x["route"] == "range_partition_utf8"]
b = [x for x in lines if x["route"] != "range_partition_utf8"]
assert all(x["counts"] == a[0]["counts"] for x in lines), "the two routes disagree"
med = lambda xs: float(np.median(xs))  # noqa: E731
summary = {"rows": N, "splitters": 7, "bytes": int(offs[-1]),
           "range_partition_utf8_call_ms_median": med([x["call_ms"] for x in a]),
           "range_partition_utf8_id_pass_kernel_ms_median": med([x["id_pass_kernel_ms"] for x in a]),
           "dictionary_route_call_ms_median": med([x["call_ms"] for x in b]),
           "dictionary_route_encode_ms_median": med([x["encode_ms"] for x in b]),
           "dictionary_route_range_partition_ms_median": med([x["range_partition_ms"] for x in b])}
print(json.dumps(summary), flush=True)
if len(sys.argv) > 1:  # the raw lines and the summary, e.g. profiles/dist_keys/range_partition_utf8_vs_dict_raw.jsonl
    with open(sys.argv[1], "w") as f:
        for x in lines + [summary]:
            f.write(json.dumps(x) + "\n")
ctx.close()
