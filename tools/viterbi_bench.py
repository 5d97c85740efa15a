#!/usr/bin/env python3
"""Time the K=7 Viterbi decoder's kernel (k_viterbi, viterbi_kernels.hip).

    python tools/viterbi_bench.py [--steps 10] [--warmup 2] [--codewords 8192] [--bytes 4798]

Workload: 8192 codewords of 4798 bytes (2398 message bytes each; the size of
BASELINE config 5's per-stream byte budget), 2 % of the coded bits inverted,
256 distinct codewords repeated over the batch.  The GPU part runs in a child
process of its own under a time limit.  Timing: HIP events on the null stream
around `steps` calls of amr_viterbi_decode_device on device-resident input,
after the warm-up calls.  One JSON line: ms per call, decoded MB/s (message
bytes out), coded Mbit/s (coded bits in), trellis steps per second, and the
parity of a 64-codeword sample -- bytes and metrics -- against the numpy
restatement (tests/viterbi_cases.py), checked before timing.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-modem-radio_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

CHILD_LIMIT_S = 420
DISTINCT = 256
SAMPLE = 64
BER = 0.02


def make_rows(n_bytes: int, seed: int):
    """DISTINCT noisy codewords of n_bytes each: (messages, rows [DISTINCT][n_bytes] uint8)."""
    import viterbi_cases as vc
    cases = vc.noisy(seed, [(n_bytes - 2) // 2] * DISTINCT, BER)
    rows = np.stack([np.frombuffer(rx, np.uint8) for _, rx in cases])
    return [m for m, _ in cases], rows


def child(B: int, L: int, steps: int, warmup: int) -> int:
    import _amr
    import viterbi_cases as vc
    assert vc.is_codeword_len(L), "--bytes must be a codeword length (even, >= 2)"
    _amr.require_gpu()
    lib = _amr.lib()
    _amr.check(lib.amr_set_device(_amr.default_device()))
    hip = ctypes.CDLL("libamdhip64.so")
    n_msg = (L - 2) // 2
    ocap = max(1, n_msg)
    wb = int(lib.amr_viterbi_work_bytes(L, B))
    msgs, tile = make_rows(L, seed=1)
    bufs = []

    def dmalloc(nbytes):
        p = ctypes.c_void_p()
        _amr.check(lib.amr_malloc(ctypes.byref(p), max(1, nbytes)))
        bufs.append(p)
        return p

    def hipcheck(rc, what):
        if rc != 0:
            raise RuntimeError(f"{what}: hip error {rc}")

    try:
        d_in, d_len, d_out = dmalloc(B * L), dmalloc(B * 8), dmalloc(B * ocap)
        d_oln, d_met, d_work = dmalloc(B * 8), dmalloc(B * 4), dmalloc(wb)
        for r0 in range(0, B, DISTINCT):
            k = min(DISTINCT, B - r0)
            _amr.check(lib.amr_memcpy_h2d(ctypes.c_void_p(d_in.value + r0 * L), _amr.ptr(tile), k * L))
        lens = np.full(B, L, np.int64)
        _amr.check(lib.amr_memcpy_h2d(d_len, _amr.ptr(lens), lens.nbytes))

        def step():
            _amr.check(lib.amr_viterbi_decode_device(None, d_in, L, d_len, B, d_out, ocap, d_oln, d_met, d_work, wb))

        for _ in range(max(1, warmup)):
            step()
        _amr.check(lib.amr_device_synchronize())
        out = np.zeros((B, ocap), np.uint8)
        met = np.zeros(B, np.int32)
        oln = np.zeros(B, np.int64)
        _amr.check(lib.amr_memcpy_d2h(_amr.ptr(out), d_out, out.nbytes))
        _amr.check(lib.amr_memcpy_d2h(_amr.ptr(met), d_met, met.nbytes))
        _amr.check(lib.amr_memcpy_d2h(_amr.ptr(oln), d_oln, oln.nbytes))
        ns = min(SAMPLE, B, DISTINCT)
        want = vc.decode_batch([tile[i].tobytes() for i in range(ns)])
        same = sum(int(out[i, :oln[i]].tobytes() == want[i][0] and int(met[i]) == want[i][1]) for i in range(ns))
        corrected = sum(int(want[i][0] == msgs[i]) for i in range(ns))
        last = B - 1                                        # the batch repeats the tile: its last row too
        tail_ok = out[last, :oln[last]].tobytes() == out[last % DISTINCT, :oln[last % DISTINCT]].tobytes()
        assert same == ns and tail_ok, f"GPU decode differs from the restatement ({same} of {ns} equal)"

        ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
        hipcheck(hip.hipEventCreate(ctypes.byref(ev0)), "hipEventCreate")
        hipcheck(hip.hipEventCreate(ctypes.byref(ev1)), "hipEventCreate")
        hipcheck(hip.hipEventRecord(ev0, None), "hipEventRecord")
        for _ in range(steps):
            step()
        hipcheck(hip.hipEventRecord(ev1, None), "hipEventRecord")
        hipcheck(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
        ms = ctypes.c_float()
        hipcheck(hip.hipEventElapsedTime(ctypes.byref(ms), ev0, ev1), "hipEventElapsedTime")
        hip.hipEventDestroy(ev0)
        hip.hipEventDestroy(ev1)
        dt = ms.value / 1e3 / steps
    finally:
        for p in bufs:
            lib.amr_free(p)
    T = 4 * L - 2
    print(json.dumps({"codewords": B, "coded_bytes": L, "message_bytes": n_msg, "ber": BER, "steps": steps,
                      "ms_per_call": round(dt * 1e3, 3), "decoded_MBps": round(B * n_msg / dt / 1e6, 1),
                      "coded_Mbitps": round(B * (16 * n_msg + 12) / dt / 1e6, 1),
                      "trellis_Gsteps_per_s": round(B * T / dt / 1e9, 3), "work_bytes": wb,
                      "parity_sample": f"{same}/{ns}", "sample_corrected": f"{corrected}/{ns}"}), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--codewords", type=int, default=8192)
    ap.add_argument("--bytes", type=int, default=4798)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.codewords, a.bytes, a.steps, a.warmup)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--warmup",
                            str(a.warmup), "--codewords", str(a.codewords), "--bytes", str(a.bytes)],
                           timeout=CHILD_LIMIT_S)
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": f"time limit of {CHILD_LIMIT_S} s"}), flush=True)
        return 124                                          # nothing more is started on the GPU after a hang
    if r.returncode != 0:
        print(json.dumps({"error": f"exit status {r.returncode}"}), flush=True)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
