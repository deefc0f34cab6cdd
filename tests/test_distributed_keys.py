"""Utf8 and temporal keys across ranks: qeh_range_partition_utf8 (csrc/k_partition.hip) against a host
model, and the distributed GROUP BY, window, sort and join of qe_hip/distributed.py with Utf8 and
temporal keys.  The multi-process cases run tests/dist_keys_worker.py: ranks share GPU 0 over gloo.

The host model of the range partition is Python's order on `bytes` (byte-wise unsigned, a proper
prefix first): ascending ids are bisect_left(splitters, s), descending ids len(splitters) -
bisect_right(splitters, s), NULL rows 0.  Every comparison is exact."""
import ctypes as C
import os
import re
import socket
import subprocess
import sys
from bisect import bisect_left, bisect_right

import numpy as np
import pytest

import qe_hip
from qe_hip import abi

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
        procs.append(subprocess.Popen([sys.executable, os.path.join(HERE, "dist_keys_worker.py"), mode], env=env,
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
    m = re.search(r"^\s*int\s+qeh_range_partition_utf8\s*\(([^)]*)\)\s*;", code, flags=re.M)
    assert m, "qeh_range_partition_utf8 is not declared in include/qeh.h"
    args = [" ".join(a.split()) for a in m.group(1).split(",")]
    assert args == ["qeh_ctx *ctx", "const qeh_column *key", "int ascending", "const int32_t *splitter_offsets",
                    "const uint8_t *splitter_bytes", "int n_splitters", "int64_t *counts", "qeh_column *out_perm"], args
    assert "qeh_range_partition_utf8" in abi.SIGNATURES
    restype, argtypes = abi.SIGNATURES["qeh_range_partition_utf8"]
    assert restype is C.c_int and len(argtypes) == 8
    lib = qe_hip.load()
    assert hasattr(lib, "qeh_range_partition_utf8")
    out = subprocess.run(["nm", "-D", "--defined-only", abi.LIB_PATH], capture_output=True, text=True).stdout
    assert re.search(r"\bqeh_range_partition_utf8\b", out)
    assert hasattr(qe_hip.Context, "range_partition_utf8")
    assert lib.qeh_abi_version() == 1


# ---- qeh_range_partition_utf8 alone ------------------------------------------------------------------

LENGTHS = [0, 1, 63, 64, 65, 257, 100_003]
SPLITTER_COUNTS = [0, 1, 2, 7, 255]
WORDS = [("w%02d" % i) * (1 + i % 4) + "abcdefghijklmnop"[:i % 17] for i in range(50)]
CHAIN = [b"ab", b"ab\x00", b"ab\x00\x00", b"abc", b""]


def population(kind, n, seed):
    """n rows of one population, as bytes."""
    r = np.random.default_rng(seed)
    if kind == "vocab":  # 50 ASCII words: heavy duplication
        return [WORDS[i].encode() for i in r.integers(0, len(WORDS), n)]
    if kind == "bytes":  # random bytes of length 0..20 with 0x00 and bytes >= 0x80
        alphabet = np.array([0, 0, 1, 0x41, 0x7F, 0x80, 0x81, 0xC3, 0xFE, 0xFF], np.uint8)
        lens = r.integers(0, 21, n)
        raw = alphabet[r.integers(0, len(alphabet), int(lens.sum()))].tobytes()
        cum = np.concatenate([[0], np.cumsum(lens)])
        return [raw[cum[i]:cum[i + 1]] for i in range(n)]
    if kind == "shared":  # the first 8, 16 or 17 bytes shared, a difference only after them
        stem = b"the-same-17-bytes"
        tails = [b"", b"\x00", b"a", b"a\x00", b"b", b"\x80", b"\xff", b"ab", b"abcdefgh", b"abcdefgi", b"abcdefgh\x00"]
        cut = np.array([8, 16, 17])[r.integers(0, 3, n)]
        t = r.integers(0, len(tails), n)
        return [stem[:cut[i]] + tails[t[i]] for i in range(n)]
    if kind == "chain":  # proper-prefix chains
        return [CHAIN[i] for i in r.integers(0, len(CHAIN), n)]
    raise ValueError(kind)


def splitter_sets(rows, seed):
    """Splitters of every count drawn from the rows (so many rows equal one), sorted; drawing 255
    from few distinct strings repeats neighbours, and one set repeats them on purpose."""
    r = np.random.default_rng(seed)
    pool = rows if rows else [b"", b"m"]
    out = [sorted(pool[i] for i in r.integers(0, len(pool), k)) for k in SPLITTER_COUNTS]
    two = sorted(pool[i] for i in r.integers(0, len(pool), 2))
    out.append([two[0], two[0], two[0], two[1], two[1]])
    return out


def model_ids(rows, valid, splitters, asc):
    if asc:
        ids = np.array([bisect_left(splitters, s) for s in rows], np.int64)
    else:
        ids = np.array([len(splitters) - bisect_right(splitters, s) for s in rows], np.int64)
    ids = ids.reshape(len(rows))
    return ids if valid is None else np.where(valid, ids, 0)


def check_partition(ctx, col, ids, n_split, what):
    counts, perm = ctx.range_partition_utf8(col, what[0], what[1])
    assert counts.dtype == np.int64 and len(counts) == n_split + 1, what[2:]
    assert np.array_equal(counts, np.bincount(ids, minlength=n_split + 1)), (what[2:], counts[:8])
    assert perm.dtype == abi.DT_UINT32 and len(perm) == len(ids) and not perm.c.validity, what[2:]
    pv, _ = perm.to_numpy()
    want = np.argsort(ids, kind="stable")
    bad = np.nonzero(pv.astype(np.int64) != want)[0]
    assert len(bad) == 0, (what[2:], bad[:4], pv[bad[:4]], want[bad[:4]])


def check_population(ctx, rows, seed, what, validities=("none", "quarter", "all")):
    n = len(rows)
    r = np.random.default_rng(seed)
    masks = {"none": None, "quarter": r.random(n) > 0.25, "all": np.zeros(n, bool)}
    sets = splitter_sets(rows, seed + 1)
    raw = {(j, asc): model_ids(rows, None, sp, asc) for j, sp in enumerate(sets) for asc in (True, False)}
    for vname in validities:
        valid = masks[vname]
        col = ctx.upload(list(rows), valid) if n else ctx.upload(np.array([], dtype=object))
        for j, sp in enumerate(sets):
            for asc in (True, False):
                ids = raw[(j, asc)] if valid is None else np.where(valid, raw[(j, asc)], 0)
                check_partition(ctx, col, ids, len(sp), (sp, asc, what, n, vname, len(sp)))
        # the order is the local sort's: along sort_indices the ids never decrease, NULLs first in partition 0
        if n:
            for asc in (True, False):
                p = ctx.sort_indices([col], [asc]).to_numpy()[0].astype(np.int64)
                for j in (3, 4):
                    ids = raw[(j, asc)] if valid is None else np.where(valid, raw[(j, asc)], 0)
                    assert (np.diff(ids[p]) >= 0).all(), (what, n, vname, asc, j)
                if valid is not None:
                    nn = int(n - valid.sum())
                    assert not valid[p[:nn]].any() and valid[p[nn:]].all(), (what, n, vname, asc)


@pytest.mark.gpu
@pytest.mark.parametrize("n", LENGTHS)
def test_range_partition_utf8_vs_host_model(ctx, n):
    """Every population at length n, splitter counts 0, 1, 2, 7, 255 and a set with repeated
    neighbours, no bitmap / 25 % NULL / all NULL, both directions, and the agreement with
    qeh_sort_indices.  The two large populations cover the multi-block grid."""
    kinds = ("vocab", "bytes") if n > 1000 else ("vocab", "bytes", "shared", "chain")
    for q, kind in enumerate(kinds):
        check_population(ctx, population(kind, n, 31 * n + q), 7 * n + q, kind,
                         validities=("none", "quarter") if n > 1000 else ("none", "quarter", "all"))


@pytest.mark.gpu
def test_range_partition_utf8_prefix_chains_as_splitters(ctx):
    """b"ab" < b"ab\\0" < b"ab\\0\\0" < b"abc", the empty string before all: as rows and as splitters."""
    rows = CHAIN * 13 + [b"a", b"abd", b"ab\x00\x01", b"\x00"]
    for sp in (sorted(CHAIN), sorted(CHAIN)[1:], [b"ab\x00"], [b"", b""], sorted(CHAIN * 2)):
        for asc in (True, False):
            check_partition(ctx, ctx.upload(list(rows)), model_ids(rows, None, sp, asc), len(sp), (sp, asc, "chain", sp))


def kib_splitters():
    """255 distinct 1 KiB splitters (255 KiB: more than a compute unit's LDS): groups of 16 share
    everything but byte 1001, the groups differ in their first byte."""
    return [bytes([1 + j // 16]) + b"x" * 1000 + bytes([0x70 + j % 16]) + b"y" * 22 for j in range(255)]


@pytest.mark.gpu
def test_range_partition_utf8_splitters_beyond_lds(ctx):
    sp = kib_splitters()
    assert sp == sorted(sp) and all(len(s) == 1024 for s in sp) and len(set(sp)) == 255
    r = np.random.default_rng(5)
    rows = []
    for j, how in zip(r.integers(0, 255, 3000), r.integers(0, 6, 3000)):
        s = sp[j]
        if how == 1:
            s = s[:int(r.integers(0, 1025))]  # a proper prefix
        elif how == 2:
            s = s + b"\x00"
        elif how == 3:
            s = s[:1001] + bytes([s[1001] + int(r.integers(-1, 2))]) + s[1002:]
        elif how == 4:
            s = s[:1023] + bytes([int(r.integers(0, 256))])
        elif how == 5:
            s = bytes([int(r.integers(0, 256))]) + s[1:]
        rows.append(s)
    valid = r.random(len(rows)) > 0.25
    for v in (None, valid):
        col = ctx.upload(list(rows), v)
        for asc in (True, False):
            check_partition(ctx, col, model_ids(rows, v, sp, asc), len(sp), (sp, asc, "1 KiB splitters", v is None))
    # the same rows against splitters that fit the LDS budget: the other home of the bytes
    few = sp[::37]
    for asc in (True, False):
        check_partition(ctx, col, model_ids(rows, valid, few, asc), len(few), (few, asc, "1 KiB splitters, 7 of them"))


@pytest.mark.gpu
def test_range_partition_utf8_sliced_from_a_poisoned_parent(ctx):
    """A slice at a non-zero offset: the parent's rows around it and the bytes its NULL slots keep
    are other strings."""
    import sliced
    r = np.random.default_rng(9)
    n = 1000
    vals = np.array([WORDS[i] + ("é" if i % 3 == 0 else "") for i in r.integers(0, len(WORDS), n)], dtype=object)
    valid = r.random(n) > 0.25
    rows = [s.encode() for s in vals]
    for lead in (3, 67):
        for v in (valid, None):
            c = sliced.make(vals, v, lead=lead)
            col = c.dev(ctx)
            assert col.c.offset == lead and len(col) == n
            for sp in splitter_sets(rows, lead)[2:]:
                for asc in (True, False):
                    check_partition(ctx, col, model_ids(rows, v, sp, asc), len(sp), (sp, asc, "sliced", lead, len(sp)))


@pytest.mark.gpu
def test_range_partition_utf8_errors_and_launch_count(ctx):
    rows = population("vocab", 1000, 3)
    col = ctx.upload(list(rows))
    sp = splitter_sets(rows, 4)[3]
    ctx.timing(True)
    ctx.timing_reset()
    ctx.range_partition_utf8(col, sp, True)
    launches = ctx.kernel_time("range_partition_utf8")[1]
    ctx.timing(False)
    assert launches == 1  # the id pass streams the column once: no dictionary

    def status(fn):
        with pytest.raises(abi.QehError) as e:
            fn()
        return e.value.status, e.value.message
    assert status(lambda: ctx.range_partition_utf8(col, [b"b", b"a"]))[0] == abi.QEH_E_INVALID
    assert status(lambda: ctx.range_partition_utf8(col, [b"ab\x00", b"ab"]))[0] == abi.QEH_E_INVALID
    assert status(lambda: ctx.range_partition_utf8(col, [b"a\xff", b"a\x7f"]))[0] == abi.QEH_E_INVALID  # unsigned bytes
    assert status(lambda: ctx.range_partition_utf8(col, [b"a"] * 256))[0] == abi.QEH_E_INVALID
    for other in (ctx.upload(np.arange(10, dtype=np.int64)), ctx.upload(np.arange(10, dtype=np.float64)),
                  ctx.upload(np.arange(10, dtype=np.int32), dtype=abi.DT_DATE32)):
        s, msg = status(lambda: ctx.range_partition_utf8(other, [b"a"]))
        assert s == abi.QEH_E_UNSUPPORTED and "qeh_range_partition" in msg.replace("qeh_range_partition_utf8", "")
    # raw calls
    lib = ctx.lib
    I32P, U8P = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
    offs = (C.c_int32 * 3)(0, 1, 2)
    data = (C.c_uint8 * 8)(97, 98)
    counts = (C.c_int64 * 3)()
    out = abi.QehColumn()
    key = C.byref(col.c)
    assert lib.qeh_range_partition_utf8(ctx.h, key, 1, offs, data, 2, counts, C.byref(out)) == abi.QEH_OK
    assert out.length == len(rows) and sum(counts) == len(rows)
    abi.check(lib.qeh_column_release(ctx.h, C.byref(out)))
    assert lib.qeh_range_partition_utf8(None, key, 1, offs, data, 2, counts, C.byref(out)) == abi.QEH_E_INVALID
    assert lib.qeh_range_partition_utf8(ctx.h, None, 1, offs, data, 2, counts, C.byref(out)) == abi.QEH_E_INVALID
    assert lib.qeh_range_partition_utf8(ctx.h, key, 1, I32P(), data, 2, counts, C.byref(out)) == abi.QEH_E_INVALID
    assert lib.qeh_range_partition_utf8(ctx.h, key, 1, offs, U8P(), 2, counts, C.byref(out)) == abi.QEH_E_INVALID
    assert lib.qeh_range_partition_utf8(ctx.h, key, 1, offs, data, 2, None, C.byref(out)) == abi.QEH_E_INVALID
    assert lib.qeh_range_partition_utf8(ctx.h, key, 1, offs, data, 2, counts, None) == abi.QEH_E_INVALID
    assert lib.qeh_range_partition_utf8(ctx.h, key, 1, offs, data, -1, counts, C.byref(out)) == abi.QEH_E_INVALID
    assert lib.qeh_range_partition_utf8(ctx.h, key, 1, offs, data, 256, counts, C.byref(out)) == abi.QEH_E_INVALID
    for bad in ((1, 1, 2), (0, 2, 1)):  # not starting at 0; decreasing
        assert lib.qeh_range_partition_utf8(ctx.h, key, 1, (C.c_int32 * 3)(*bad), data, 2, counts,
                                            C.byref(out)) == abi.QEH_E_INVALID
    # no splitters: one partition, the identity permutation; a null bytes pointer is fine with no byte to read
    zero = (C.c_int32 * 1)(0)
    assert lib.qeh_range_partition_utf8(ctx.h, key, 0, zero, U8P(), 0, counts, C.byref(out)) == abi.QEH_OK
    assert counts[0] == len(rows)
    abi.check(lib.qeh_column_release(ctx.h, C.byref(out)))


# ---- the distributed operators (ranks as processes on one GPU) ---------------------------------------
# Worlds 1 and 3 run DistributedExecutor(ctx), the host-staged path; world 2 runs every case on both
# that and DistributedExecutor(ctx, device="cuda").

WORLDS = [1, 2, 3]


@pytest.mark.gpu
@pytest.mark.parametrize("world", WORLDS)
def test_group_by_utf8_keys(world):
    """5 000 + 17 * rank rows per rank; keys [Utf8], [Utf8, Int64], [Int64, Utf8]; 97 strings with "é",
    "ß", "日本", the empty string, a pair that differs after byte 8 and one on rank 0 only; NULL keys;
    SUM(Int64), COUNT, MIN, AVG(Float64, 20 % NULL).  Then two groups job-wide, and rank 1 empty."""
    launch("group_by", world)


@pytest.mark.gpu
@pytest.mark.parametrize("world", WORLDS)
def test_windows_with_utf8_keys(world):
    """ROW_NUMBER, RANK and LAG(v, 2, default) PARTITION BY Utf8 ORDER BY Int64, and PARTITION BY
    Int64 ORDER BY Utf8 DESC: each rank's result is its slice of the single-device result."""
    launch("window", world)


@pytest.mark.gpu
@pytest.mark.parametrize("world", WORLDS)
def test_sort_by_utf8_keys(world):
    """ORDER BY Utf8 and ORDER BY Utf8 DESC, Int64 with 10 % NULL keys and a row-id payload; one
    string everywhere, three distinct strings, all-NULL keys, rank 1 empty."""
    launch("sort", world)


@pytest.mark.gpu
@pytest.mark.parametrize("world", WORLDS)
def test_hash_join_inner_on_utf8_keys(world):
    """2 000 build rows per rank with duplicates and NULLs, 5 000 probe rows with about 30 % unmatched:
    the joined rows of all ranks are the single-device qeh_hash_join's, as a multiset."""
    launch("join", world)


@pytest.mark.gpu
@pytest.mark.parametrize("world", WORLDS)
def test_temporal_keys_and_payloads(world):
    """GROUP BY Date32 / Timestamp(us), ORDER BY Timestamp(us) DESC, ROW_NUMBER PARTITION BY Date32
    ORDER BY Timestamp(ns), a join on Date64, and an exchange carrying Date32 / Timestamp(ms)
    payloads: values, NULLs and dtypes."""
    launch("temporal", world)


@pytest.mark.gpu
@pytest.mark.parametrize("world", WORLDS)
def test_remaining_refusals_are_raised_on_every_rank(world):
    """What stays QEH_E_UNSUPPORTED raises on every rank before a collective (the launcher's time
    limit is the guard against a hang)."""
    launch("refusals", world)
