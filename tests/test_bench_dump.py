"""bench.py --dump-outputs on the host: what bench.dump_outputs writes for a
step's outputs (float32 / float64 .npy files, bytes past a stream's length
zeroed, a fixed seeded sample of rows once the arrays pass the size budget)."""
import os

import numpy as np


def _step_outputs(rows, cap, seed=3):
    rng = np.random.default_rng(seed)
    return {"bytes": rng.integers(1, 256, (rows, cap)).astype(np.uint8),       # no zero: padding is visible
            "lengths": rng.integers(0, cap + 1, rows).astype(np.int64),
            "sync_idx": rng.integers(-1, 1 << 40, rows).astype(np.int64)}


def test_dump_whole_output(tmp_path):
    import bench
    host = _step_outputs(37, 11)
    host["lengths"][:2] = (0, 11)
    written = bench.dump_outputs(str(tmp_path / "d"), host, {"bytes": "lengths"})
    assert sorted(written) == ["bytes.npy", "lengths.npy", "rows.npy", "sync_idx.npy"]
    got = {k[:-4]: np.load(tmp_path / "d" / k) for k in written}
    assert got["bytes"].dtype == np.float32 and got["lengths"].dtype == np.float64 and got["sync_idx"].dtype == np.float64
    assert np.array_equal(got["rows"], np.arange(37))
    assert np.array_equal(got["lengths"], host["lengths"]) and np.array_equal(got["sync_idx"], host["sync_idx"])
    for i in range(37):
        n = host["lengths"][i]
        assert np.array_equal(got["bytes"][i, :n], host["bytes"][i, :n]) and not got["bytes"][i, n:].any()
    assert written["bytes.npy"] == [37, 11]


def test_dump_samples_rows_within_budget(tmp_path):
    import bench
    host = _step_outputs(500, 64)
    budget = 20000
    w1 = bench.dump_outputs(str(tmp_path / "a"), host, {"bytes": "lengths"}, budget=budget)
    bench.dump_outputs(str(tmp_path / "b"), _step_outputs(500, 64), {"bytes": "lengths"}, budget=budget)
    size = sum(np.load(tmp_path / "a" / k).nbytes for k in w1)
    assert 0.9 * budget <= size <= budget
    rows = np.load(tmp_path / "a" / "rows.npy").astype(int)
    assert 0 < rows.size < 500 and np.all(np.diff(rows) > 0)
    assert np.array_equal(np.load(tmp_path / "a" / "lengths.npy"), host["lengths"][rows])
    for k in w1:                                          # the same sample and bytes from run to run
        assert open(os.path.join(tmp_path, "a", k), "rb").read() == open(os.path.join(tmp_path, "b", k), "rb").read()
