"""Window functions against the plain-Python model (tests/window_model.py) on three grids, all exact:
integer results by value, value results by bits and validity, no tolerance anywhere.

Every case runs twice: on the CPU the C oracle against the model (not marked gpu: this proves the
inputs and the model), on the GPU the device against the model.  C = kBlock * kRnPer, the sorted
path's chunk (k_window_sort.hip), read from the sources so a changed tile moves the shapes with it.

(a) Key shapes, C + 17 rows, the default (sorted) path.  One case per (n_part, n_order) in (0,0) (0,1)
    (0,2) (1,0) (1,1) (1,2) (2,1) (2,2) (4,4) and per direction pattern (all ascending, all descending,
    alternating; one pattern where there is no ORDER BY key): 23 cases.  The key columns come from the
    pool Int32, Int64, Float32, Float64, Bool, Utf8, Date32, Timestamp(us), taken cyclically from a
    start that moves with the case, and each key is non-nullable, ~10 % NULL or all-NULL, cycled the
    same way (the STARTS table); test_key_grid_covers_the_pool asserts that every (type, nullability,
    role) occurs.  Keys hold 2 to 6 distinct values (Bool has two; the floats need six for +-0.0, +-inf and two NaN
    payloads), and every row is drawn from a third as many base rows, so partitions, peer groups and
    full-tuple ties all occur; some partitions are one peer group with the same ORDER BY tuple as the
    next partition's, so that only the partition flag separates their peers.  Each case runs
    ROW_NUMBER through qeh_row_number and qeh_window, RANK, DENSE_RANK, NTILE(3), LAG and LEAD with and
    without a default, FIRST_VALUE and LAST_VALUE; the argument type (Int32, Int64, Float32, Float64,
    with NULLs) cycles with the case.  Also: 5 keys on either side, and columns of unequal lengths.
(b) Layouts, 3C + 17 rows, one Int64 PARTITION BY and one Int64 ORDER BY key built so that the sorted
    order has prescribed partition and peer starts (L1..L7 below), scattered by a fixed permutation,
    L3 also in exactly reversed input order; each also with a NULL first partition key and a NULL
    first peer group in every partition.  The construction is checked through the model's order.
    The non-null layouts run again under QEH_WINDOW_MSD=1 and QEH_WINDOW_MSD=1 + QEH_WINDOW_W3=1
    with the ORDER BY column as the argument (what those paths accept).  On the CPU the two switches
    share one case, their inputs being the same.
(c) Parameter edges on L3 and L6, and on L7, whose partitions are small enough for the partitioning
    paths to take, all three paths: NTILE bucket counts and LAG / LEAD offsets around the partition
    size, the chunk, 2^31, 2^32 and 2^63 - 1, with and without a default.
"""
import os
import re

import numpy as np
import pytest

import oracle_bind as ob
import window_model as wm
from qe_hip import abi
from qe_hip.plan import WindowFunctionType as W

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "query-engine_amd", "csrc")


def _const(source, name):
    with open(os.path.join(CSRC, source)) as f:
        return int(re.search(r"constexpr int %s = (\d+);" % name, f.read()).group(1))


K_BLOCK = _const("device_common.h", "kBlock")
C = K_BLOCK * _const("k_window_sort.hip", "kRnPer")  # sorted positions per chunk of the max-scans
FUNC_NAME = {v: k for k, v in vars(W).items() if not k.startswith("_")}


# ---- columns and the three executors -------------------------------------------------------------
class Col:
    """A test column: numpy values (a list of str for Utf8; physical integers for temporal types),
    validity or None, and the temporal dtype if any."""

    def __init__(self, values, valid=None, temporal=None):
        self.values, self.valid, self.temporal = values, valid, temporal

    def model(self):
        return self.values, self.valid

    def oracle(self):
        v = self.values
        if isinstance(v, list):  # the oracle has no Utf8 keys: the strings' rank codes, in byte order
            live = [s.encode() for i, s in enumerate(v) if self.valid is None or self.valid[i]]
            code = {s: i for i, s in enumerate(sorted(set(live)))}
            v = np.array([code[s.encode()] if self.valid is None or self.valid[i] else 0 for i, s in enumerate(v)],
                         np.int32)
        return ob.HostCol(v, self.valid)

    def device(self, ctx):
        return ctx.upload(self.values, self.valid, dtype=self.temporal)


class Runner:
    """One window's inputs on the oracle (ctx None) or the device; run() gives (values, validity-or-None)."""

    def __init__(self, ctx, part, order, asc, arg, arg_is_order=False):
        self.ctx, self.asc, self.n = ctx, asc, len((part + order + [arg])[0].values)
        conv = (lambda c: c.device(ctx)) if ctx is not None else (lambda c: c.oracle())
        self.part, self.order = [conv(c) for c in part], [conv(c) for c in order]
        self.arg = self.order[0] if arg_is_order else conv(arg)

    def run(self, func, param=0, default=None, row_number_api=False):
        need_arg = func >= W.Lag or not (self.part or self.order)  # OVER (): the argument gives the row count
        if self.ctx is None:
            if row_number_api:
                return ob.row_number(self.part, self.order, self.asc), None
            return ob.window(func, self.part, self.order, self.asc, arg=self.arg if func >= W.Lag else None,
                             param=param, default=default, n=self.n)
        if row_number_api:
            return self.ctx.row_number(self.part, self.order, self.asc).to_numpy()
        return self.ctx.window(func, self.part, self.order, self.asc, arg=self.arg if need_arg else None,
                               param=param, default=default).to_numpy()


def _model(func, part, order, asc, arg, param, default):
    return wm.window(func, [c.model() for c in part], [c.model() for c in order], asc,
                     arg=arg.model() if arg is not None else None, param=param, default=default)


def _assert_same(func, got, want, label):
    gv, gm = got
    wv, wok = want
    if func < W.Lag:
        assert gm is None or gm.all(), label
        assert np.array_equal(gv, np.array(wv, np.int64)), label
        return
    gm = np.ones(len(gv), bool) if gm is None else gm
    assert np.array_equal(gm, np.array(wok, bool)), label
    u = {4: np.uint32, 8: np.uint64}[gv.dtype.itemsize]
    wv = np.array([v if ok else 0 for v, ok in zip(wv, wok)], gv.dtype)
    assert np.array_equal(gv.view(u)[gm], wv.view(u)[gm]), label


# (function, param, with default, through qeh_row_number): all eight functions
CALLS = [(W.RowNumber, 0, False, True), (W.RowNumber, 0, False, False), (W.Rank, 0, False, False),
         (W.DenseRank, 0, False, False), (W.Ntile, 3, False, False), (W.Lag, 1, False, False), (W.Lag, 2, True, False),
         (W.Lead, 2, False, False), (W.Lead, 1, True, False), (W.FirstValue, 0, False, False),
         (W.LastValue, 0, False, False)]


def _check_calls(runner, part, order, asc, arg, default, calls=CALLS, after=None):
    for func, param, with_default, api in calls:
        if api and not (part or order):
            continue  # qeh_row_number takes at least one key
        label = "%s(%d)%s%s" % (FUNC_NAME[func], param, " default" if with_default else "", " row_number api" if api else "")
        d = default if with_default else None
        a = arg if func >= W.Lag or not (part or order) else None
        want = _model(func, part, order, asc, a, param, d)
        if after is not None:
            after(None, label)  # reset the timing records
        _assert_same(func, runner.run(func, param, d, api), want, label)
        if after is not None:
            after(func, label)


# ---- (a) key shapes ------------------------------------------------------------------------------
N_KEYS = C + 17
POOL = ["i32", "i64", "f32", "f64", "bool", "utf8", "date32", "ts_us"]
MODES = ["not null", "some null", "all null"]
ARGS = ["i32", "i64", "f32", "f64"]
DEFAULTS = {"i32": -7, "i64": -(2 ** 40) - 3, "f32": float("nan"), "f64": -0.0}
F32 = np.array([0x80000000, 0, 0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00123], np.uint32).view(np.float32)
F64 = np.array([1 << 63, 0, 0x7FF << 52, 0xFFF << 52, 0x7FF8 << 48, (0xFFF8 << 48) | 0x123], np.uint64).view(np.float64)
CANDIDATES = {
    "i32": (np.array([-(2 ** 31), -1, 7, 2 ** 31 - 1], np.int32), None),
    "i64": (np.array([-(2 ** 63), 0, 5, 2 ** 63 - 1], np.int64), None),
    "f32": (F32, None),  # -0.0, +0.0, +inf, -inf and two NaN payloads (one with the sign set)
    "f64": (F64, None),
    "bool": (np.array([False, True]), None),
    "utf8": (["", "ab", "abc", "b"], None),  # the empty string and a shared prefix
    "date32": (np.array([-719162, -1, 0, 19000], np.int32), abi.DT_DATE32),
    "ts_us": (np.array([-(2 ** 62), -1, 0, 1_700_000_000_000_000], np.int64), abi.DT_TIMESTAMP_US),
}
SHAPES = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 1), (2, 2), (4, 4)]
# per case: where its keys start in POOL and in MODES, chosen so that the 23 cases cover every
# (type, nullability, role) and only p1o0 has nothing but all-NULL PARTITION BY keys (one partition);
# test_key_grid_covers_the_pool holds the table to that
STARTS = [(4, 0), (0, 1), (6, 2), (3, 0), (1, 0), (2, 1), (7, 2), (4, 2), (5, 0), (7, 1), (1, 1), (4, 1), (0, 0), (2, 0),
          (7, 0), (6, 1), (3, 2), (5, 2), (6, 0), (2, 2), (1, 2), (0, 2), (5, 1)]
KEY_CASES = []  # (n_part, n_order, direction pattern, pool start, mode start, argument type)
for _p, _o in SHAPES:
    for _d in (["asc", "desc", "alt"] if _o else ["asc"]):
        _i = len(KEY_CASES)
        KEY_CASES.append((_p, _o, _d) + STARTS[_i] + (ARGS[_i % 4],))


def _case_keys(case):
    """[(role, type, mode)] of a case's key columns, PARTITION BY keys first."""
    n_part, n_order, _, start, m0, _ = case
    return [("part" if j < n_part else "order", POOL[(start + j) % 8], MODES[(m0 + j) % 3]) for j in range(n_part + n_order)]


def _key_case_data(case):
    n_part, n_order, dirs, _, _, argkind = case
    r = np.random.default_rng(KEY_CASES.index(case))
    m = N_KEYS // 3
    src = r.integers(0, m, N_KEYS)  # every row repeats one of m base rows: full-tuple ties, NULLs included
    keys = _case_keys(case)
    draws = [r.integers(0, len(CANDIDATES[kind][0]), m) for _, kind, _ in keys]
    live = [r.random(m) > 0.1 for _ in keys]  # used by the ~10 % NULL keys
    # Partitions whose rows are all peers, next to one another with the same ORDER BY tuple (only the
    # partition flag separates their peer groups): where the first PARTITION BY key that is not all-NULL
    # holds one of the lower half of its values (both of a Bool's), every ORDER BY key holds its first value.
    lead = next((j for j in range(n_part) if keys[j][2] != "all null"), None)
    if lead is not None:
        flat = draws[lead] < max(2, len(CANDIDATES[keys[lead][1]][0]) // 2)  # two partitions at least
        if keys[lead][2] == "some null":
            flat &= live[lead]
        for j in range(n_part, n_part + n_order):
            draws[j][flat], live[j][flat] = 0, True
    cols = []
    for (_, kind, mode), draw, ok in zip(keys, draws, live):
        cand, temporal = CANDIDATES[kind]
        draw = draw[src]
        values = [cand[d] for d in draw] if isinstance(cand, list) else cand[draw]
        valid = {"not null": None, "some null": ok[src], "all null": np.zeros(N_KEYS, bool)}[mode]
        cols.append(Col(values, valid, temporal))
    asc = [{"asc": True, "desc": False, "alt": j % 2 == 0}[dirs] for j in range(n_order)]
    if argkind in ("i32", "i64"):
        a = r.integers(-(2 ** 31), 2 ** 31, N_KEYS).astype(np.int32 if argkind == "i32" else np.int64)
        if argkind == "i64":
            a *= 2 ** 31 + 11
    else:
        a = np.round(r.standard_normal(N_KEYS), 2).astype(np.float32 if argkind == "f32" else np.float64)
        a[::7] = (F32 if argkind == "f32" else F64)[np.arange(len(a[::7])) % 6]
    arg = Col(a, r.random(N_KEYS) > 0.2)
    return cols[:n_part], cols[n_part:], asc, arg, DEFAULTS[argkind]


def _key_id(case):
    return "p%do%d-%s" % case[:3]


def test_key_grid_covers_the_pool():
    seen = {k for case in KEY_CASES for k in _case_keys(case)}
    assert seen == {(role, t, m) for role in ("part", "order") for t in POOL for m in MODES}
    assert {case[5] for case in KEY_CASES} == set(ARGS)
    one_partition = [_key_id(c) for c in KEY_CASES if c[0] and all(k[2] == "all null" for k in _case_keys(c)[:c[0]])]
    assert one_partition == ["p1o0-asc"]


PARTITIONED_AND_ORDERED = [c for c in KEY_CASES if c[1] and any(k[0] == "part" and k[2] != "all null" for k in _case_keys(c))]


@pytest.mark.parametrize("case", PARTITIONED_AND_ORDERED, ids=_key_id)
def test_key_grid_has_partitions_sharing_an_order_tuple(case):
    """Where one partition ends and the next begins with the same ORDER BY tuple, only the partition
    flag tells their peer groups apart: every case with an ORDER BY key and a PARTITION BY key that
    is not all-NULL has such a place."""
    part, order, asc, _, _ = _key_case_data(case)
    key = wm.row_keys([c.model() for c in part], [c.model() for c in order], asc, N_KEYS)
    rows = wm.sorted_rows([c.model() for c in part], [c.model() for c in order], asc, N_KEYS)
    n_part = len(part)
    assert any(key[a][:n_part] != key[b][:n_part] and key[a][n_part:] == key[b][n_part:] for a, b in zip(rows, rows[1:]))


@pytest.mark.parametrize("case", KEY_CASES, ids=_key_id)
def test_key_shapes_oracle(case):
    part, order, asc, arg, default = _key_case_data(case)
    _check_calls(Runner(None, part, order, asc, arg), part, order, asc, arg, default)


@pytest.mark.gpu
@pytest.mark.parametrize("case", KEY_CASES, ids=_key_id)
def test_key_shapes_device(ctx, monkeypatch, case):
    monkeypatch.delenv("QEH_WINDOW_MSD", raising=False)
    part, order, asc, arg, default = _key_case_data(case)
    _check_calls(Runner(ctx, part, order, asc, arg), part, order, asc, arg, default)


@pytest.mark.gpu
def test_key_count_and_length_errors(ctx):
    """5 keys on either side: UNSUPPORTED.  Keys of different lengths, or an argument of another
    length than the keys: INVALID."""
    import qe_hip
    k, short = ctx.upload(np.arange(8, dtype=np.int64)), ctx.upload(np.arange(7, dtype=np.int64))

    def status(call):
        with pytest.raises(qe_hip.QehError) as e:
            call()
        return e.value.status

    for func in (W.Rank, W.Lag):
        assert status(lambda: ctx.window(func, [k] * 5, [k], [True], arg=k, param=1)) == abi.QEH_E_UNSUPPORTED
        assert status(lambda: ctx.window(func, [k], [k] * 5, [True] * 5, arg=k, param=1)) == abi.QEH_E_UNSUPPORTED
        assert status(lambda: ctx.window(func, [k, short], [k], [True], arg=k, param=1)) == abi.QEH_E_INVALID
        assert status(lambda: ctx.window(func, [k], [k, short], [True] * 2, arg=k, param=1)) == abi.QEH_E_INVALID
        assert status(lambda: ctx.window(func, [k], [short], [True], arg=k, param=1)) == abi.QEH_E_INVALID
    assert status(lambda: ctx.window(W.Lead, [k], [k], [True], arg=short, param=1)) == abi.QEH_E_INVALID
    assert status(lambda: ctx.window(W.RowNumber, [k] * 5, [k], [True])) == abi.QEH_E_UNSUPPORTED
    assert status(lambda: ctx.row_number([k] * 5, [k], [True])) == abi.QEH_E_UNSUPPORTED
    assert status(lambda: ctx.row_number([k, short], [k], [True])) == abi.QEH_E_INVALID


# ---- (b) layouts -----------------------------------------------------------------------------------
N = 3 * C + 17


def _every(starts, step):
    """Peer starts: every `step`-th place of each partition (its start included)."""
    flag = np.zeros(N, bool)
    flag[list(starts)] = True
    pos = np.arange(N)
    first = np.maximum.accumulate(np.where(flag, pos, 0))
    return set(pos[(pos - first) % step == 0].tolist())


def _l7_starts():
    sizes, starts, at = [63, 64, 65, K_BLOCK - 1, K_BLOCK, K_BLOCK + 1], [], 0
    while at < N:
        starts.append(at)
        at += sizes[(len(starts) - 1) % len(sizes)]
    return set(starts)


def layout_starts(name):
    """(partition starts, peer-group starts) as sets of sorted positions."""
    everything = set(range(N))
    if name == "L1":  # one partition, one peer group: every chunk after the first has no flag at all
        return {0}, {0}
    if name == "L2":  # one partition, all order keys distinct
        return {0}, everything
    if name == "L3":  # partition starts on and around the chunk edges
        p = {0, C - 1, C, C + 1, 2 * C, 2 * C + 1}
        return p, _every(p, 3)
    if name == "L4":  # every row its own partition
        return everything, everything
    if name == "L5":  # one partition from position 1; a peer group from C-1 to 2C+1 spans a whole chunk
        return {0, 1}, set(range(C)) | set(range(2 * C + 2, N))
    if name == "L6":  # one-row first and last partitions around one big partition
        p = {0, 1, N - 1}
        return p, _every(p, 5)
    p = _l7_starts()  # L7: partition sizes 63, 64, 65, kBlock-1, kBlock, kBlock+1, repeated
    return p, _every(p, 2)


LAYOUTS = ["L1", "L2", "L3", "L4", "L5", "L6", "L7"]
SCATTER = np.random.default_rng(7).permutation(N)


def _layout_data(name, nullable=False, reverse=False):
    """(partition key, order key, argument with NULLs) whose window order has layout_starts(name)."""
    ps, qs = layout_starts(name)
    pos = np.arange(N)
    fp, fq = np.isin(pos, list(ps)), np.isin(pos, list(qs))
    pid = np.cumsum(fp) - 1                     # partition index of a sorted position
    peer = np.cumsum(fq) - np.cumsum(fq)[np.maximum.accumulate(np.where(fp, pos, 0))]  # peer group in the partition
    at = (N - 1 - pos) if reverse else SCATTER  # sorted position i sits at input row at[i]
    k, v = np.empty(N, np.int64), np.empty(N, np.int64)
    k[at], v[at] = pid * 3 - 7, peer * 2 - 5
    km = vm = None
    if nullable:  # NULLs sort first: the first partition's key and every partition's first peer group
        km, vm = np.empty(N, bool), np.empty(N, bool)
        km[at], vm[at] = pid != 0, peer != 0
        k[~km], v[~vm] = 2 ** 40, -(2 ** 40)    # what lies under a NULL must not matter
    r = np.random.default_rng(len(ps) + len(qs))
    arg = Col(r.standard_normal(N), r.random(N) > 0.2)
    return Col(k, km), Col(v, vm), arg


LAYOUT_CASES = [(name, nullable, False) for name in LAYOUTS for nullable in (False, True)] + [("L3", False, True)]
MSD_LAYOUT_CASES = [c for c in LAYOUT_CASES if not c[1]]  # the partitioning paths take non-null keys


def _layout_id(case):
    return case[0] + ("-nullable" if case[1] else "") + ("-reversed" if case[2] else "")


@pytest.mark.parametrize("case", LAYOUT_CASES, ids=_layout_id)
def test_layout_construction(case):
    """The model's sorted order has exactly the intended partition and peer starts."""
    k, v, _ = _layout_data(*case)
    rows = np.array(wm.sorted_rows([k.model()], [v.model()], [True], N))
    assert sorted(rows.tolist()) == list(range(N))

    def changes(cols):  # sorted positions whose (validity, value) differs from the row before
        f = np.zeros(N, bool)
        f[0] = True
        for c in cols:
            ok = np.ones(N, bool) if c.valid is None else c.valid
            val = np.where(ok, c.values, 0)[rows]
            f[1:] |= (ok[rows][1:] != ok[rows][:-1]) | (val[1:] != val[:-1])
        return set(np.nonzero(f)[0].tolist())

    ps, qs = layout_starts(case[0])
    assert ps <= qs
    assert changes([k]) == ps
    assert changes([k, v]) == qs


@pytest.mark.parametrize("case,path",
                         [(c, "sorted") for c in LAYOUT_CASES] + [(c, "partitioning") for c in MSD_LAYOUT_CASES],
                         ids=lambda x: x if isinstance(x, str) else _layout_id(x))
def test_layouts_oracle(case, path):
    k, v, arg = _layout_data(*case)
    arg = v if path == "partitioning" else arg
    _check_calls(Runner(None, [k], [v], [True], arg), [k], [v], [True], arg, 7)


PATH_ENV = {"sorted": {}, "msd": {"QEH_WINDOW_MSD": "1"}, "w3": {"QEH_WINDOW_MSD": "1", "QEH_WINDOW_W3": "1"}}


def _set_path(monkeypatch, path):
    for name in ("QEH_WINDOW_MSD", "QEH_WINDOW_W3", "QEH_NO_WINDOW_MSD"):
        monkeypatch.delenv(name, raising=False)
    for name, value in PATH_ENV[path].items():
        monkeypatch.setenv(name, value)


def _path_watch(ctx, path, must_partition):
    """Called before (func None) and after each window call: which path ran, by its timing records."""
    def watch(func, label):
        if func is None:
            ctx.timing_reset()
            return
        partitioned = ctx.kernel_time("window_sort")[1] > 0 or ctx.kernel_time("w3_place")[1] > 0
        if path == "sorted":
            assert not partitioned, label
            assert ctx.kernel_time("row_number" if func == W.RowNumber else "window")[1] > 0, label
        elif must_partition:
            assert partitioned, label
    return watch


def _run_layout_on_device(ctx, monkeypatch, case, path, calls, default):
    _set_path(monkeypatch, path)
    k, v, arg = _layout_data(*case)
    on_order = path != "sorted"  # the partitioning paths take value functions of the order column only
    arg = v if on_order else arg
    ctx.timing(True)
    try:
        _check_calls(Runner(ctx, [k], [v], [True], arg, arg_is_order=on_order), [k], [v], [True], arg, default, calls,
                     after=_path_watch(ctx, path, case[0] in ("L4", "L7")))
    finally:
        ctx.timing(False)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LAYOUT_CASES, ids=_layout_id)
def test_layouts_device_sorted_path(ctx, monkeypatch, case):
    _run_layout_on_device(ctx, monkeypatch, case, "sorted", CALLS, 7)


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["msd", "w3"])
@pytest.mark.parametrize("case", MSD_LAYOUT_CASES, ids=_layout_id)
def test_layouts_device_partitioning_paths(ctx, monkeypatch, case, path):
    """Layouts with partitions above 2048 rows fall back and need only be right; L4 and L7 must partition."""
    _run_layout_on_device(ctx, monkeypatch, case, path, CALLS, 7)


# ---- (c) parameter edges ---------------------------------------------------------------------------
# layout -> its largest partition (L7: the layout whose partitions the partitioning paths take)
EDGE_LAYOUTS = {"L3": C + 16, "L6": N - 2, "L7": K_BLOCK + 1}


def _edge_calls(func, size):
    if func == W.Ntile:
        return [(W.Ntile, p, False, False) for p in (1, 2, size - 1, size, size + 1, C, 2 ** 31, 2 ** 32 + 1, 2 ** 63 - 1)]
    offsets = (0, 1, 63, 64, C - 1, C, C + 1, size - 1, size, 2 ** 31, 2 ** 32, 2 ** 63 - 1)
    return [(func, p, d, False) for p in offsets for d in (False, True)]


def test_edge_layouts_largest_partition():
    for name, size in EDGE_LAYOUTS.items():
        starts = sorted(layout_starts(name)[0]) + [N]
        assert max(b - a for a, b in zip(starts, starts[1:])) == size


@pytest.mark.parametrize("func", [W.Ntile, W.Lag, W.Lead], ids=FUNC_NAME.get)
@pytest.mark.parametrize("path", ["sorted", "partitioning"])
@pytest.mark.parametrize("name", sorted(EDGE_LAYOUTS))
def test_parameter_edges_oracle(name, path, func):
    k, v, arg = _layout_data(name)
    arg = v if path == "partitioning" else arg
    _check_calls(Runner(None, [k], [v], [True], arg), [k], [v], [True], arg, -9, _edge_calls(func, EDGE_LAYOUTS[name]))


@pytest.mark.gpu
@pytest.mark.parametrize("func", [W.Ntile, W.Lag, W.Lead], ids=FUNC_NAME.get)
@pytest.mark.parametrize("path", sorted(PATH_ENV))
@pytest.mark.parametrize("name", sorted(EDGE_LAYOUTS))
def test_parameter_edges_device(ctx, monkeypatch, name, path, func):
    _run_layout_on_device(ctx, monkeypatch, (name, False, False), path, _edge_calls(func, EDGE_LAYOUTS[name]), -9)


def test_bad_parameters_oracle_and_model():
    k = np.zeros(4, np.int64)
    for func, param in ((W.Ntile, 0), (W.Lag, -1), (W.Lead, -1)):
        with pytest.raises(ob.OracleError) as e:
            ob.window(func, [ob.HostCol(k)], [ob.HostCol(k)], [True], arg=ob.HostCol(k), param=param)
        assert e.value.status == abi.QEH_E_INVALID
        with pytest.raises(ValueError):
            wm.window(func, [(k, None)], [(k, None)], [True], arg=(k, None), param=param)


@pytest.mark.gpu
@pytest.mark.parametrize("path", sorted(PATH_ENV))
def test_bad_parameters_device(ctx, monkeypatch, path):
    """NTILE(0) and a negative offset keep giving INVALID on every path."""
    import qe_hip
    _set_path(monkeypatch, path)
    k = ctx.upload(np.arange(8, dtype=np.int64))
    for func, param in ((W.Ntile, 0), (W.Ntile, -(2 ** 63)), (W.Lag, -1), (W.Lead, -1), (W.Lead, -(2 ** 63))):
        with pytest.raises(qe_hip.QehError) as e:
            ctx.window(func, [k], [k], [True], arg=k, param=param)
        assert e.value.status == abi.QEH_E_INVALID, (func, param)


# ---- the model itself ------------------------------------------------------------------------------
def test_model_doc_examples():
    """The worked examples of docs/WINDOW_FUNCTIONS.md:44-205, the same ones test_oracle_doc_examples uses."""
    def col(x):
        return (x, None)

    sal = [60000, 80000, 90000, 80000]  # Alice, Charlie, Diana, Eve: ORDER BY salary DESC
    assert wm.window(wm.ROW_NUMBER, [], [col(sal)], [False])[0] == [4, 2, 1, 3]  # ties by input position
    assert wm.window(wm.RANK, [], [col(sal)], [False])[0] == [4, 2, 1, 2]        # Alice skips 3
    assert wm.window(wm.DENSE_RANK, [], [col(sal)], [False])[0] == [3, 2, 1, 2]  # no gap
    sal4 = [60000, 70000, 80000, 90000]  # Alice, Bob, Charlie, Diana
    assert wm.window(wm.ROW_NUMBER, [], [col(sal4)], [False])[0] == [4, 3, 2, 1]
    assert wm.window(wm.NTILE, [], [col(sal4)], [False], param=4)[0] == [4, 3, 2, 1]
    sales, date = [100.0, 120.0, 115.0], [1, 2, 3]  # LAG(sales, 1) OVER (ORDER BY date)
    assert wm.window(wm.LAG, [], [col(date)], [True], arg=col(sales), param=1) == ([None, 100.0, 120.0], [False, True, True])
    lead = wm.window(wm.LEAD, [], [col(date)], [True], arg=col(sales), param=1)
    assert lead == ([120.0, 115.0, None], [True, True, False])
    dept, s = ["Sales", "Eng", "Sales", "Eng", "Sales"], [10, 40, 30, 20, 30]
    assert wm.window(wm.FIRST_VALUE, [col(dept)], [col(s)], [False], arg=col(s))[0] == [30, 40, 30, 40, 30]
    assert wm.window(wm.LAST_VALUE, [col(dept)], [col(s)], [True], arg=col(s))[0] == [30, 40, 30, 40, 30]
    # RANK() OVER (PARTITION BY department ORDER BY salary DESC): Diana, Charlie (Eng), Bob, Alice (Sales)
    dep, pay = ["Eng", "Eng", "Sales", "Sales"], [90000, 80000, 70000, 60000]
    assert wm.window(wm.RANK, [col(dep)], [col(pay)], [False])[0] == [1, 2, 1, 2]


def test_model_ordering_rules():
    nan_a, nan_b = F32[4], F32[5]
    keys = (np.array([0.0, -0.0, np.inf, -np.inf, 1.0], np.float32).tolist(), None)  # python floats: binary64
    assert wm.sorted_rows([], [keys], [True], 5) == [3, 1, 0, 4, 2]       # -inf < -0.0 < +0.0 < 1 < +inf
    f32 = (np.array([nan_a, nan_b, nan_a, -0.0, 0.0], np.float32), [True, True, True, True, False])
    assert wm.sorted_rows([], [f32], [True], 5) == [4, 1, 3, 0, 2]        # NULL, -NaN, -0.0, +NaN twice
    assert wm.sorted_rows([], [f32], [False], 5) == [4, 0, 2, 3, 1]       # NULL first in both directions
    assert wm.window(wm.DENSE_RANK, [], [f32], [True])[0] == [4, 2, 4, 3, 1]
    assert wm.sorted_rows([], [(["b", "", "ab", "abc"], None)], [True], 4) == [1, 2, 3, 0]
    assert wm.sorted_rows([], [(np.array([True, False, True]), None)], [True], 3) == [1, 0, 2]
    nul = ([5, 6, 7, 8], [False, True, False, True])                      # NULLs are one partition, and peers
    assert wm.window(wm.ROW_NUMBER, [nul], [], [])[0] == [1, 1, 2, 1]
    assert wm.window(wm.RANK, [], [nul], [True])[0] == [1, 3, 1, 4]
    v = ([1, 2, 3], [True, False, True])
    assert wm.window(wm.LAG, [], [], [], arg=v, param=1, default=-1) == ([-1, 1, None], [True, True, False])
    assert wm.window(wm.LEAD, [], [], [], arg=v, param=2 ** 63 - 1) == ([None] * 3, [False] * 3)


def test_model_ntile_against_explicit_buckets():
    """NTILE(n): n buckets in order, the first size % n one row larger, built row by row."""
    for size in range(1, 23):
        for n in list(range(1, 26)) + [2 ** 31, 2 ** 63 - 1]:
            q, r = divmod(size, n)
            want = [b + 1 for b in range(min(n, size)) for _ in range(q + (b < r))]
            assert [wm.ntile(i, size, n) for i in range(size)] == want, (size, n)
