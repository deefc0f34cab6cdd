"""Sliced (non-zero Arrow offset) inputs for the operator tests of test_sliced_inputs.py.

`make()` builds a logical column together with a poisoned parent: `lead` rows before it and TRAIL
rows after it hold values and validity bits that change any answer which includes them.  `Col.dev`
uploads the parent at offset 0 and returns `ctx.slice(parent, lead, n)`, so the view has a non-zero
offset and, with a validity buffer, an unknown NULL count.  `Col.view` gives the host the logical
rows or one of three mis-sliced readings of the parent (the mistakes a kernel can make).

`Host` and `Dev` run one operator through the CPU oracle (or a numpy restatement where the oracle has
no entry point) and through the device, and return plain (values, validity) pairs; `ordered` and
`multiset` turn those into a canonical matrix that compares exactly (floats by their bits)."""
import os
import sys
import zlib

import numpy as np

import oracle_bind as ob
from qe_hip import abi

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import pg_text  # noqa: E402

LEADS = (1, 2, 8, 67)
TRAIL = 200
# the leads of one call's columns, by the lead that names the case: 2 and 8 keep every 8-byte column
# 16-B aligned (the fast paths stay on); 1 and 67 mix odd and aligned columns in one call
CYCLES = {1: (1, 2, 67, 8), 2: (2, 8), 8: (8, 2), 67: (67, 8, 1, 2)}


def lead_cycle(lead):
    cyc = CYCLES[lead]
    state = {"i": 0}

    def nxt():
        state["i"] += 1
        return cyc[(state["i"] - 1) % len(cyc)]
    return nxt


def is_utf8(v):
    return isinstance(v, np.ndarray) and v.dtype == object


class Col:
    """A logical column (values, valid-or-None) inside its poisoned parent."""

    def __init__(self, values, valid, lead, pvalues, pvalid, table):
        self.values, self.valid, self.lead, self.pvalues, self.pvalid, self.table = values, valid, lead, pvalues, pvalid, table
        self.n = len(values)

    def view(self, mode="ok"):
        n, L = self.n, self.lead
        if mode == "ok":
            return self.values, self.valid
        if mode == "a":  # values from parent rows [0, n)
            return self.pvalues[:n], self.valid
        if mode == "b":  # validity read from bit 0
            return self.values, self.pvalid[:n]
        if mode == "c":  # one row past the end
            return self.pvalues[L:L + n + 1], None if self.pvalid is None else self.pvalid[L:L + n + 1]
        raise ValueError(mode)

    def dev(self, ctx, sliced=True):
        if not sliced:
            if is_utf8(self.values):
                return upload_utf8(ctx, self.values, self.valid)
            return ctx.upload(self.values, self.valid)
        if is_utf8(self.pvalues):
            parent = upload_utf8(ctx, self.pvalues, self.pvalid)
        else:
            parent = ctx.upload(self.pvalues, self.pvalid)
        return ctx.slice(parent, self.lead, self.n)


def upload_utf8(ctx, strs, valid):
    """Utf8 column whose NULL rows keep their bytes and whose validity buffer exists whenever
    `valid` is given (Context.upload drops an all-valid one)."""
    enc = [s.encode() for s in strs]
    n = len(enc)
    offs = np.zeros(n + 1, np.int32)
    offs[1:] = np.cumsum([len(b) for b in enc])
    data = np.frombuffer(b"".join(enc) + b"\0" * 8, np.uint8)
    po, pd = ctx.alloc(offs.nbytes), ctx.alloc(data.nbytes)
    ctx.h2d(po, offs)
    ctx.h2d(pd, data)
    c = abi.QehColumn(dtype=abi.DT_UTF8, owned=0, length=n, offset=0, null_count=0, values=pd, offsets=po,
                      values_bytes=int(offs[-1]))
    bufs = [po, pd]
    if valid is not None:
        from qe_hip.device import pack_bits
        vb = pack_bits(valid)
        q = ctx.alloc(vb.nbytes)
        ctx.h2d(q, vb)
        c.validity = q
        c.null_count = int(n - np.asarray(valid, bool).sum())
        bufs.append(q)
    from qe_hip.device import DeviceColumn
    return DeviceColumn(ctx, c, bufs)


def make(values, valid=None, lead=1, key=False, inside=False, table=0, poison=None):
    """values: numpy array (object dtype = Utf8).  valid: None (no validity buffer), a bool array, or
    "buffer" (all valid, but a validity buffer is there).  key: integer poison stays within twice the
    logical range (a direct table's key range must not overflow).  inside: integer poison is taken
    from the logical values only (row-id columns, which index other columns).  poison: the poison
    values themselves, cycled (where only certain values change the answer, as in IN's set)."""
    values = np.asarray(values)
    n = len(values)
    if isinstance(valid, str):
        valid = np.ones(n, bool)
    elif valid is not None:
        valid = np.asarray(valid, bool)
    m = lead + TRAIL
    idx = np.arange(m)
    exist = values[(idx * 7 + 3) % n]
    if poison is not None:
        poison = np.asarray(poison)[idx % len(poison)]
        poison = np.concatenate([poison[:lead], poison[:TRAIL]]).astype(values.dtype)
    elif is_utf8(values):
        poison = np.array(["poison-%04d-" % i + "x" * (40 + i % 5) for i in range(m)], dtype=object)
    elif values.dtype == np.bool_:
        poison = np.concatenate([~values[np.arange(lead) % n], ~values[::-1][np.arange(TRAIL) % n][::-1]])
    elif values.dtype.kind == "f":
        poison = np.array([np.nan, np.inf, -np.inf, -0.0], values.dtype)[idx % 4]
    elif inside:
        poison = exist.copy()
    elif key:
        live = values if valid is None else values[valid]
        lo, hi = int(live.min()), int(live.max())
        half = (hi - lo + 1) // 2 + 1
        # an existing key first: the row next to the slice on either side repeats a key of the slice
        poison = np.where(idx % 3 == 0, exist, np.where(idx % 3 == 1, lo - half, hi + half)).astype(values.dtype)
        poison = np.concatenate([poison[:lead], poison[:TRAIL]])
    else:
        info = np.iinfo(values.dtype)
        poison = np.where(idx % 3 == 0, info.min, np.where(idx % 3 == 1, info.max, exist)).astype(values.dtype)
        poison = np.concatenate([poison[:lead], poison[:TRAIL]])
    pvalues = np.concatenate([poison[:lead], values, poison[lead:]])
    if is_utf8(values):
        pvalues = pvalues.astype(object)
    pvalid = None
    if valid is not None:
        pvalid = np.concatenate([np.full(lead, not valid[0]), valid, np.full(TRAIL, not valid[-1])])
    return Col(values, valid, lead, pvalues, pvalid, table)


# ---- canonical results ------------------------------------------------------------------------------

def _bits(v):
    v = np.asarray(v)
    if v.dtype == object:
        return np.array([zlib.crc32(s.encode() if isinstance(s, str) else bytes(s)) + (len(s) << 32) for s in v], np.int64)
    if v.dtype.kind == "M":
        return v.view(np.int64)
    if v.dtype == np.float64:
        return v.view(np.int64)
    if v.dtype == np.float32:
        return v.view(np.int32).astype(np.int64)
    return v.astype(np.int64)


class Canon:
    def __init__(self, cols, sort):
        self.kinds = []
        rows = []
        n = None
        for v, m in cols:
            v = np.asarray(v)
            n = len(v)
            m = np.ones(n, bool) if m is None else np.asarray(m, bool)
            self.kinds.append("utf8" if v.dtype == object else v.dtype.name)
            rows += [m.astype(np.int64), np.where(m, _bits(v), 0)]
        self.mat = np.stack(rows) if rows else np.zeros((0, 0), np.int64)
        if sort and rows and n:
            self.mat = self.mat[:, np.lexsort(self.mat[::-1])]

    def __eq__(self, other):
        return self.mat.shape == other.mat.shape and np.array_equal(self.mat, other.mat)

    def diff(self, other):
        if self.mat.shape != other.mat.shape:
            return "shape %s vs %s" % (self.mat.shape, other.mat.shape)
        bad = np.argwhere(self.mat != other.mat)
        if len(bad) == 0:
            return "equal"
        r, c = bad[0]
        return "%d cells differ; first: column %d (%s) %s row %d: %d vs %d" % (
            len(bad), r // 2, self.kinds[r // 2], "value" if r % 2 else "validity", c, self.mat[r, c], other.mat[r, c])


def ordered(cols):
    return Canon(cols, False)


def multiset(cols):
    return Canon(cols, True)


def plain(a):
    """one array with no validity as a column"""
    return np.asarray(a), None


# ---- the two backends -------------------------------------------------------------------------------

def hash64(k):
    """device_common.h hash64 (murmur3 fmix64) over uint64 arrays"""
    k = k.astype(np.uint64)
    with np.errstate(over="ignore"):
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xff51afd7ed558ccd)
        k ^= k >> np.uint64(33)
        k *= np.uint64(0xc4ceb9fe1a85ec53)
        k ^= k >> np.uint64(33)
    return k


def _valid(p):
    return np.ones(len(p[0]), bool) if p[1] is None else np.asarray(p[1], bool)


def _stable_parts(part, n_parts):
    counts = np.bincount(part, minlength=n_parts).astype(np.int64)
    return counts, np.argsort(part, kind="stable").astype(np.int64)


def _codes(p):
    """a Utf8 pair as Int64 ranks in byte order (a sort or join on them is one on the strings)"""
    v, m = p
    if not is_utf8(v):
        return p
    enc = np.array([s.encode() for s in v], dtype=object)
    _, inv = np.unique(enc, return_inverse=True)
    return inv.astype(np.int64), m


def _take_pair(p, idx):
    v, m = p
    return np.asarray(v)[idx], None if m is None else np.asarray(m)[idx]


class Host:
    """The reference: the CPU oracle, or numpy where the oracle has no such entry point.  Columns are
    (values, valid-or-None) pairs."""
    gpu = False

    def col(self, c, mode="ok"):
        return c.view(mode)

    @staticmethod
    def H(p):
        return ob.HostCol(*_codes(p))

    def hash_aggregate(self, keys, inputs, aggs):
        wk, wa, g, _ = ob.hash_aggregate([self.H(k) for k in keys], [self.H(c) for c in inputs], aggs)
        return list(wk), list(wa)

    def filter_aggregate(self, cols, pred, key_idx, aggs):
        hc = [self.H(c) for c in cols]
        if pred is not None:
            fc, _, _ = ob.filter(hc, pred)
            hc = [ob.HostCol(v, m) for v, m in fc]
        wk, wa, g, _ = ob.hash_aggregate([hc[i] for i in key_idx], hc, aggs)
        return list(wk), list(wa)

    def filter(self, cols, pred, out_idx, max_rows=None):
        """the oracle picks the rows (Utf8 columns stand in as codes); the columns are gathered here"""
        n = len(cols[0][0])
        fc, _, _ = ob.filter([self.H(c) for c in cols] + [ob.HostCol(np.arange(n, dtype=np.int64))], pred, out_idx=[len(cols)])
        rows = fc[0][0][:max_rows]
        return [(np.asarray(cols[j][0])[rows], _valid(cols[j])[rows]) for j in out_idx]

    def columns_minmax(self, cols):
        out = []
        for v, m in cols:
            live = np.asarray(v)[_valid((v, m))].astype(np.int64)
            out.append((int(live.min()), int(live.max()), len(live)))
        return np.array(out, np.int64)

    def utf8_dict_encode(self, c):
        enc = np.array([s.encode() for s in c[0]], dtype=object)
        m = _valid(c)
        dic, inv = np.unique(enc[m], return_inverse=True)
        codes = np.zeros(len(enc), np.int32)
        codes[m] = inv
        return (codes, m), (np.array([b.decode() for b in dic], dtype=object), None)

    def join_utf8(self, jt, lk, lcols, rk, rcols):
        """Utf8 keys as codes of one dictionary over both sides"""
        both = np.array([s.encode() for s in np.concatenate([lk[0], rk[0]])], dtype=object)
        _, inv = np.unique(both, return_inverse=True)
        cl, cr = (inv[:len(lk[0])].astype(np.int64), lk[1]), (inv[len(lk[0]):].astype(np.int64), rk[1])
        return self.join_inner(cl, lcols, cr, rcols) if jt == 0 else self.join_outer(jt, cl, lcols, cr, rcols)

    def join_filter_aggregate(self, probe, kidx, pred, bk, gks, aggs):
        wk, wa, g = ob.join_filter_aggregate([self.H(c) for c in probe], kidx, pred, self.H(bk), [self.H(c) for c in gks], aggs)
        return list(wk), list(wa)

    def join_inner(self, pk, pcols, bk, bcols):
        wp, wb, _ = ob.hash_join_inner(self.H(pk), [self.H(c) for c in pcols], self.H(bk), [self.H(c) for c in bcols])
        return wp + wb

    def join_outer(self, jt, lk, lcols, rk, rcols):
        wl, wr, _ = ob.hash_join_outer(jt, self.H(lk), [self.H(c) for c in lcols], self.H(rk), [self.H(c) for c in rcols])
        return wl + wr

    def sort_indices(self, keys, asc):
        return ob.sort_indices([self.H(k) for k in keys], asc).astype(np.int64)

    def sort_indices_nulls(self, keys, asc, nf):
        return ob.sort_indices_nulls([self.H(k) for k in keys], asc, nf).astype(np.int64)

    def sort_indices_limit(self, keys, asc, limit):
        return self.sort_indices(keys, asc)[:limit]

    def row_number(self, part, order, asc):
        return ob.row_number([self.H(c) for c in part], [self.H(c) for c in order], asc)

    def window(self, func, part, order, asc, arg=None, param=0, default=None):
        return ob.window(func, [self.H(c) for c in part], [self.H(c) for c in order], asc,
                         arg=None if arg is None else self.H(arg), param=param, default=default)

    def hash_partition(self, key, parts):
        v, m = key
        part = np.where(_valid(key), (hash64(np.asarray(v).astype(np.int64).view(np.uint64)) % np.uint64(parts)).astype(np.int64), 0)
        return _stable_parts(part, parts)

    def range_partition(self, key, split, asc):
        from qe_hip.device import order_keys
        okey = order_keys(key[0])
        split = np.asarray(split, np.int64)
        part = (split[None, :] < okey[:, None]).sum(1) if asc else (split[None, :] > okey[:, None]).sum(1)
        return _stable_parts(np.where(_valid(key), part, 0), len(split) + 1)

    def _perm(self, keys, parts):
        counts, perm = ob.partition_hash([self.H(k) for k in keys], parts)
        return counts.astype(np.int64), perm.astype(np.int64)

    def partition_hash_move(self, keys, parts, cols):
        counts, perm = self._perm(keys, parts)
        return counts, [_take_pair(c, perm) for c in cols]

    def partition_hash_unmove(self, key, parts, moved):
        _, perm = self._perm([key], parts)
        out = []
        for v, m in moved:
            o = np.empty_like(np.asarray(v))
            o[perm] = v
            out.append((o, None))
        return out

    def filter_partition_hash_move(self, cols, pred, kidx, parts, move):
        fc, _, _ = ob.filter([self.H(c) for c in cols], pred, out_idx=[kidx] + list(move))
        counts, perm = ob.partition_hash([ob.HostCol(fc[0][0])], parts)
        return counts.astype(np.int64), [(v[perm], None) for v, _ in fc[1:]]

    def take(self, col, idx):
        return _take_pair(col, np.asarray(idx[0]).astype(np.int64))

    def scatter(self, col, perm):
        p = np.asarray(perm[0]).astype(np.int64)
        out = np.zeros(int(p.max()) + 1, np.asarray(col[0]).dtype)
        out[p] = col[0]
        return out, None

    def concat(self, parts):
        v = np.concatenate([np.asarray(p[0]) for p in parts])
        if any(is_utf8(p[0]) for p in parts):
            v = v.astype(object)
        return v, np.concatenate([_valid(p) for p in parts])

    def merge_sorted(self, parts, key_idx, asc, nf, numpy=False):
        whole = [self.concat([p[j] for p in parts]) for j in range(len(parts[0]))]
        if numpy:  # one integer key: numpy's stable lexsort, NULLs before or after every value
            (kv, km), = [whole[i] for i in key_idx]
            kv = np.where(km, np.asarray(kv).astype(np.int64), 0)  # NULL rows tie: they keep their order
            perm = np.lexsort((kv if asc[0] else -kv, km if nf[0] else ~km))
        else:
            perm = self.sort_indices_nulls([whole[i] for i in key_idx], asc, nf)
        return [_take_pair(c, perm) for c in whole]

    def avg_finalize(self, s, cnt, input_dtype):
        sv = np.asarray(s[0])
        v = sv.astype(np.int32).astype(np.float64) if input_dtype == abi.DT_INT32 else sv.astype(np.float64)
        if s[1] is not None:
            v = np.where(s[1], v, 0.0)
        c = np.asarray(cnt[0])
        valid = (c > 0) & _valid(cnt)
        with np.errstate(all="ignore"):
            return v / c.astype(np.float64), valid

    def in_set(self, probe, sset, negated):
        pk, pm = _bits(probe[0]), _valid(probe)
        sk, sm = _bits(sset[0]), _valid(sset)
        n = len(pk)
        if len(sk) == 0:
            return np.full(n, bool(negated)), np.ones(n, bool)
        hit = np.isin(pk, sk[sm])
        has_null = not sm.all()
        valid = pm & (hit | (not has_null))
        return np.where(hit, not negated, bool(negated)), valid

    def eval(self, cols, expr):
        (vals, valid), _ = ob.eval_expr([self.H(c) for c in cols], expr, len(cols[0][0]))
        return vals, valid

    def encode_pg_datarows(self, cols):
        def kind(v):
            return "utf8" if is_utf8(v) else {"bool": "bool"}.get(np.asarray(v).dtype.name, np.asarray(v).dtype.name)
        rows = pg_text.encode_rows([(kind(v), [None if (m is not None and not m[i]) else v[i] for i in range(len(v))])
                                    for v, m in cols])
        return np.array(rows, dtype=object), None

    def encode_arrow_ipc(self, cols, names):
        return [(np.asarray(v), _valid((v, m))) for v, m in cols]


class Dev:
    """The device through qe_hip.Context; columns are DeviceColumns, results come back as pairs."""
    gpu = True

    def __init__(self, ctx, sliced=True):
        self.ctx, self.sliced = ctx, sliced

    def col(self, c, mode="ok"):
        return c.dev(self.ctx, self.sliced)

    @staticmethod
    def out(cols):
        return [c.to_numpy() for c in cols]

    def hash_aggregate(self, keys, inputs, aggs):
        gk, ga, g = self.ctx.hash_aggregate(keys, inputs, aggs)
        return self.out(gk), self.out(ga)

    def filter_aggregate(self, cols, pred, key_idx, aggs):
        gk, ga, g = self.ctx.filter_aggregate(cols, pred, key_idx, aggs)
        return self.out(gk), self.out(ga)

    def join_filter_aggregate(self, probe, kidx, pred, bk, gks, aggs):
        gk, ga, g = self.ctx.join_filter_aggregate(probe, kidx, pred, bk, gks, aggs)
        return self.out(gk), self.out(ga)

    def join_inner(self, pk, pcols, bk, bcols):
        op, obd, rows = self.ctx.hash_join_inner(pk, pcols, bk, bcols)
        got = self.out(op + obd)
        assert all(len(v) == rows for v, _ in got)
        return got

    def join_outer(self, jt, lk, lcols, rk, rcols):
        ol, orr, rows = self.ctx.hash_join_outer(jt, lk, lcols, rk, rcols)
        got = self.out(ol + orr)
        assert all(len(v) == rows for v, _ in got)
        return got

    def filter(self, cols, pred, out_idx, max_rows=None):
        out, rows = self.ctx.filter(cols, pred, out_idx, max_rows)
        got = self.out(out)
        assert all(len(v) == rows for v, _ in got)
        return got

    def columns_minmax(self, cols):
        return np.array(self.ctx.columns_minmax(cols), np.int64)

    def utf8_dict_encode(self, c):
        codes, dic = self.ctx.utf8_dict_encode(c)
        return codes.to_numpy(), dic.to_numpy()

    def join_utf8(self, jt, lk, lcols, rk, rcols):
        ol, orr, rows = self.ctx.hash_join(jt, lk, lcols, rk, rcols)
        got = self.out(ol + orr)
        assert all(len(v) == rows for v, _ in got)
        return got

    def _ids(self, c):
        v, m = c.to_numpy()
        assert m is None or m.all()
        return v.astype(np.int64)

    def sort_indices(self, keys, asc):
        return self._ids(self.ctx.sort_indices(keys, asc))

    def sort_indices_nulls(self, keys, asc, nf):
        return self._ids(self.ctx.sort_indices_nulls(keys, asc, nf))

    def sort_indices_limit(self, keys, asc, limit):
        return self._ids(self.ctx.sort_indices_limit(keys, asc, limit))

    def row_number(self, part, order, asc):
        return self._ids(self.ctx.row_number(part, order, asc))

    def window(self, func, part, order, asc, arg=None, param=0, default=None):
        v, m = self.ctx.window(func, part, order, asc, arg=arg, param=param, default=default).to_numpy()
        return v, (np.ones(len(v), bool) if m is None else m)

    def hash_partition(self, key, parts):
        counts, perm = self.ctx.hash_partition(key, parts)
        return counts, self._ids(perm)

    def range_partition(self, key, split, asc):
        counts, perm = self.ctx.range_partition(key, split, asc)
        return counts, self._ids(perm)

    def partition_hash_move(self, keys, parts, cols):
        counts, moved = self.ctx.partition_hash_move(keys, parts, cols)
        return counts, self.out(moved)

    def partition_hash_unmove(self, key, parts, moved):
        # the moved columns are made on the device by the move of the same (sliced) key
        return self.out(self.ctx.partition_hash_unmove(key, parts, moved))

    def filter_partition_hash_move(self, cols, pred, kidx, parts, move):
        counts, moved = self.ctx.filter_partition_hash_move(cols, pred, kidx, parts, move)
        return counts, self.out(moved)

    def take(self, col, idx):
        return self.ctx.take(col, idx).to_numpy()

    def scatter(self, col, perm):
        return self.ctx.scatter(col, perm).to_numpy()

    def concat(self, parts):
        return self.ctx.concat(parts).to_numpy()

    def merge_sorted(self, parts, key_idx, asc, nf, numpy=False):
        cols, rows = self.ctx.merge_sorted(parts, key_idx, asc, nf)
        return self.out(cols)

    def avg_finalize(self, s, cnt, input_dtype):
        return self.ctx.avg_finalize(s, cnt, input_dtype).to_numpy()

    def in_set(self, probe, sset, negated):
        return self.ctx.in_set(probe, sset, negated).to_numpy()

    def eval(self, cols, expr):
        out = self.ctx.eval(cols, expr)
        return (out[0] if isinstance(out, tuple) else out).to_numpy()

    def encode_pg_datarows(self, cols):
        return np.array(self.ctx.encode_pg_datarows(cols).to_bytes(), dtype=object), None

    def encode_arrow_ipc(self, cols, names):
        import pyarrow as pa
        t = pa.ipc.open_stream(pa.py_buffer(self.ctx.encode_arrow_ipc(cols, names))).read_all()
        assert t.schema.names == list(names)
        out = []
        for c in t.columns:
            a = c.combine_chunks()
            valid = ~np.asarray(a.is_null().to_numpy(zero_copy_only=False), bool)
            if pa.types.is_string(a.type):
                vals = np.array([x if x is not None else "" for x in a.to_pylist()], dtype=object)
            elif pa.types.is_boolean(a.type):
                vals = np.asarray(a.fill_null(False).to_numpy(zero_copy_only=False), bool)
            else:
                vals = np.asarray(a.fill_null(0).to_numpy(zero_copy_only=False))
            out.append((vals, valid))
        return out
