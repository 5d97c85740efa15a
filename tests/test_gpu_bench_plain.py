"""A plain bench.py run (no --full) at small sizes: the line holds the headline
and `ms_per_step` over exactly --steps steps and none of the --full legs, and
--dump-outputs writes the last timed step's outputs as float32 / float64 .npy
files.  The headline layout, and the fused-FEC workload with two steps per
launch and a partial last launch (3 steps)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("parity", "cpu_baseline", "roofline", "sustained", "workloads", "dropin", "host_path_pcie_inclusive",
             "latency_ms_one_batch", "kernel_ms_solo")


@pytest.mark.parametrize("extra,rows,names", [
    (["--batch", "192"], 192, {"bytes", "lengths", "sync_idx", "rows"}),
    (["--workload", "psk8fec", "--batch", "160", "--coalesce", "2"], 160,
     {"bytes", "lengths", "sync_idx", "fec_bytes", "fec_lengths", "fec_ok", "rows"})])
def test_plain_run_and_dump(tmp_path, extra, rows, names):
    out = tmp_path / "dump"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--samples", "24000", "--dump-outputs", str(out), *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["full"] is False and d["higher_is_better"] is True
    assert d["unit"] == "Msym/s" and d["dtype"] == "f64" and d["metric"]
    sym = d["config"]["global_batch"] * d["config"]["symbols_per_stream"]
    assert d["ms_per_step"] > 0 and d["value"] == pytest.approx(sym / d["ms_per_step"] / 1e3, rel=1e-3)
    assert not [k for k in FULL_ONLY if k in d]
    got = {f[:-4]: np.load(out / f) for f in os.listdir(out)}
    assert set(got) == names == {k[:-4] for k in d["dumped_outputs"]}
    assert sum(a.nbytes for a in got.values()) <= 64e6
    assert all(a.dtype in (np.float32, np.float64) and a.shape[0] == rows for a in got.values())
    assert np.array_equal(got["rows"], np.arange(rows))
    for b, ln in (("bytes", "lengths"), ("fec_bytes", "fec_lengths")):
        if b not in got:
            continue
        n = got[ln].astype(int)
        assert n.min() >= 0 and n.max() <= got[b].shape[1]
        assert b != "bytes" or n.min() > 0                       # every stream demodulated something
        past = np.arange(got[b].shape[1])[None, :] >= n[:, None]
        assert not got[b][past].any() and got[b].max() <= 255 and np.array_equal(got[b], np.floor(got[b]))
        assert len({r_.tobytes() for r_ in got[b]}) > 1          # distinct noisy streams, not one row repeated
