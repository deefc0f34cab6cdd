"""bench.py's plain / --full split and --dump-outputs: what a plain run prints and writes, that the dumped
arrays are the query's result (against the oracle), and that --full still checks the result."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

ROWS, DIM, GROUPS = 300_001, 20_011, 37   # odd sizes, more than one block, every group populated
SHAPE = ["--rows", str(ROWS), "--dim", str(DIM), "--groups", str(GROUPS)]


class _Col:
    def __init__(self, vals, valid=None):
        self.vals, self.valid = np.asarray(vals), valid

    def to_numpy(self):
        return self.vals, self.valid


def test_dump_outputs_orders_by_key_and_writes_float64(tmp_path):
    keys = _Col(np.array([5, 1, 3], np.int64))
    sums = _Col(np.array([0.5, 0.25, 0.0]), np.array([True, True, False]))
    counts = _Col(np.array([50, 10, 0], np.int64))
    bench.dump_outputs(([keys], [sums, counts], 3), ["sum_v", "count_v"], str(tmp_path), 0, 1)
    got = {f: np.load(tmp_path / f) for f in sorted(os.listdir(tmp_path))}
    assert sorted(got) == ["count_v.npy", "group_key_0.npy", "sum_v.npy", "sum_v_valid.npy"]
    assert all(a.dtype == np.float64 for a in got.values())
    assert got["group_key_0.npy"].tolist() == [1.0, 3.0, 5.0]
    assert got["sum_v.npy"].tolist() == [0.25, 0.0, 0.5]
    assert got["sum_v_valid.npy"].tolist() == [1.0, 0.0, 1.0]
    assert got["count_v.npy"].tolist() == [10.0, 0.0, 50.0]
    bench.dump_outputs(([keys], [sums, counts], 3), ["sum_v", "count_v"], str(tmp_path / "r"), 1, 2)
    assert sorted(os.listdir(tmp_path / "r")) == ["count_v.rank1.npy", "group_key_0.rank1.npy", "sum_v.rank1.npy",
                                                  "sum_v_valid.rank1.npy"]


def test_dump_outputs_refuses_more_than_the_limit(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 16)
    with pytest.raises(AssertionError):
        bench.dump_outputs(([_Col(np.arange(3))], [_Col(np.zeros(3))], 3), ["sum_v"], str(tmp_path), 0, 1)
    assert os.listdir(tmp_path) == []


def _run(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *SHAPE, *extra],
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_run_dumps_the_query_result(tmp_path):
    out = tmp_path / "dump"
    line = _run("--steps", "3", "--warmup", "1", "--dump-outputs", str(out))
    assert line["steps"] == 3 and line["warmup"] == 1 and line["ms_per_step"] > 0
    assert line["unit"] == "rows/s" and line["higher_is_better"] is True and line["dtype"] == "int64/f64"
    assert line["value"] == pytest.approx(ROWS / (line["ms_per_step"] * 1e-3), rel=1e-9)
    assert line["cpu_baseline"] is None and line["result_check"].startswith("not run")
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert all(a.dtype == np.float64 and a.shape == (GROUPS,) for a in got.values())

    import oracle_bind as ob
    from qe_hip import AggregateFunction as AF, BinaryOp, abi, binop, col, lit
    x = ob.generate(abi.GEN_UNIFORM_MOD, bench.SEED, 1, ROWS, 100)
    k = ob.generate(abi.GEN_UNIFORM_MOD, bench.SEED, 2, ROWS, DIM)
    v = ob.generate(abi.GEN_UNIT_F64, bench.SEED, 3, ROWS)
    dk = ob.generate(abi.GEN_PERMUTATION, bench.SEED, 0, DIM, DIM)
    dg = ob.generate(abi.GEN_UNIFORM_MOD, bench.SEED, 5, DIM, GROUPS)
    wk, wa, wg = ob.join_filter_aggregate([ob.HostCol(x), ob.HostCol(k), ob.HostCol(v)], 1,
                                          binop(col(0), BinaryOp.Greater, lit(49)), ob.HostCol(dk), [ob.HostCol(dg)],
                                          [(AF.Sum, 2), (AF.Count, 2)])
    assert wg == GROUPS
    order = np.argsort(wk[0][0])
    assert np.array_equal(got["group_key_0"], wk[0][0][order].astype(np.float64))
    assert np.array_equal(got["count_v"], wa[1][0][order].astype(np.float64))
    assert wa[0][1] is None or wa[0][1].all()
    assert "sum_v_valid" not in got or got["sum_v_valid"].all()
    np.testing.assert_allclose(got["sum_v"], wa[0][0][order], rtol=1e-6, atol=0)  # helpers.FLOAT_RTOL


@pytest.mark.gpu
def test_full_run_checks_the_result():
    line = _run("--steps", "2", "--warmup", "1", "--full", "--cpu-sample", "0")
    assert line["steps"] == 2 and line["result_check"].endswith("passed")
    assert line["result_groups"] == GROUPS and line["result_rows_counted"] > 0
