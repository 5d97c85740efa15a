#!/usr/bin/env python3
"""Time the Hellschreiber receiver's kernel (k_hell_energy, hell_kernels.hip).

    python tools/hell_bench.py [--steps 20] [--warmup 3] [--cases f32,i16] [--no-host]

Two shapes: 4096 x 96000 float32 and 16384 x 96000 int16 (raw), default
parameters (sps 784: 122 pixels, 17 bytes per stream).  Each GPU case runs in
a child process of its own under a time limit.  Per case one JSON line:
ms per step (amr_hell_demod_device on device-resident input: the plan kernel
+ k_hell_energy, a host clock around `steps` calls ending in a device
synchronise) and the achieved GB/s against the algorithmic bytes
B * N * sizeof(T).  Beside it, unless --no-host: the reference's numpy detector
(np.mean(chunk ** 2) > 0.1 per pixel, hellschreiber.py:162-165) on one host
core, timed on a few captures and scaled to the batch.
The first stream's bytes are checked against that detector before timing.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-modem-radio_amd"))

CASES = {"f32": (4096, 96000, np.float32), "i16": (16384, 96000, np.int16)}
BAUD, FS = 122.5, 96000.0
CHILD_LIMIT_S = 240


def make_rows(rows: int, n: int, dtype, seed: int) -> np.ndarray:
    rng = np.random.default_rng(seed)
    if np.dtype(dtype) == np.float32:
        return rng.normal(0.0, 0.33, (rows, n)).astype(np.float32)       # pixel energies on both sides of 0.1
    return rng.integers(-32768, 32768, (rows, n)).astype(np.int16)


def numpy_detector(x: np.ndarray, sps: int) -> np.ndarray:
    """The reference's pixel loop on one capture."""
    with np.errstate(all="ignore"):
        return np.array([np.mean(x[i:i + sps] ** 2) > 0.1 for i in range(0, x.size - sps + 1, sps)], bool)


def child(case: str, steps: int, warmup: int) -> int:
    import _amr
    B, n, dtype = CASES[case]
    _amr.require_gpu()
    L = _amr.lib()
    _amr.check(L.amr_set_device(_amr.default_device()))
    es = np.dtype(dtype).itemsize
    elem = _amr.hell_elem(dtype)
    n_pix = int(L.amr_hell_pixels(n, BAUD, FS))
    n_out = n_pix // 7
    wb = int(L.amr_hell_work_bytes(BAUD, FS))
    bufs = []

    def dmalloc(nbytes):
        p = ctypes.c_void_p()
        _amr.check(L.amr_malloc(ctypes.byref(p), nbytes))
        bufs.append(p)
        return p

    try:
        d_x, d_out, d_len, d_work = dmalloc(B * n * es), dmalloc(B * n_out), dmalloc(B * 8), dmalloc(wb)
        tile = make_rows(256, n, dtype, seed=1)                            # 256 distinct captures, repeated
        for r0 in range(0, B, 256):
            _amr.check(L.amr_memcpy_h2d(ctypes.c_void_p(d_x.value + r0 * n * es), _amr.ptr(tile), tile.nbytes))

        def step():
            _amr.check(L.amr_hell_demod_device(None, d_x, elem, B, n, n, BAUD, FS, d_out, n_out, d_len, None, d_work, wb))

        for _ in range(max(1, warmup)):
            step()
        _amr.check(L.amr_device_synchronize())
        out = np.zeros((B, n_out), np.uint8)
        _amr.check(L.amr_memcpy_d2h(_amr.ptr(out), d_out, out.nbytes))
        lut = _amr.hell_rx_lookup()
        bits = numpy_detector(tile[0], n // n_pix)
        want = bytes(lut[sum(int(b) << i for i, b in enumerate(bits[7 * g:7 * g + 7]))] for g in range(n_out))
        assert out[0].tobytes() == want == out[256 if B > 256 else 0].tobytes(), "GPU bytes differ from the numpy detector"
        t0 = time.perf_counter()
        for _ in range(steps):
            step()
        _amr.check(L.amr_device_synchronize())
        dt = (time.perf_counter() - t0) / steps
    finally:
        for p in bufs:
            L.amr_free(p)
    nbytes = B * n * es
    print(json.dumps({"case": case, "streams": B, "samples": n, "dtype": np.dtype(dtype).name, "steps": steps,
                      "ms_per_step": round(dt * 1e3, 4), "algorithmic_bytes": nbytes,
                      "GBps": round(nbytes / dt / 1e9, 1)}), flush=True)
    return 0


def host_baseline(case: str) -> dict:
    B, n, dtype = CASES[case]
    sps = int(round(FS / BAUD))
    rows = make_rows(4, n, dtype, seed=1)
    numpy_detector(rows[0], sps)
    t0 = time.perf_counter()
    for r in rows:
        numpy_detector(r, sps)
    per = (time.perf_counter() - t0) / len(rows)
    return {"case": case, "numpy_detector_ms_per_capture": round(per * 1e3, 3),
            "numpy_detector_s_per_batch_one_core": round(per * B, 2)}


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cases", default="f32,i16")
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.steps, a.warmup)
    rc = 0
    for case in a.cases.split(","):
        if case not in CASES:
            ap.error(f"unknown case {case!r}")
        if not a.no_host:
            print(json.dumps(host_baseline(case)), flush=True)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", case, "--steps", str(a.steps),
                                "--warmup", str(a.warmup)], timeout=CHILD_LIMIT_S)
        except subprocess.TimeoutExpired:
            print(json.dumps({"case": case, "error": f"time limit of {CHILD_LIMIT_S} s"}), flush=True)
            return 124                                  # nothing more is started on the GPU after a hang
        if r.returncode != 0:
            print(json.dumps({"case": case, "error": f"exit status {r.returncode}"}), flush=True)
            return r.returncode                         # nor after a fault
        rc = rc or r.returncode
    return rc


if __name__ == "__main__":
    sys.exit(main())
