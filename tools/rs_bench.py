#!/usr/bin/env python3
"""Time the Reed-Solomon kernels (k_rs_encode, k_rs_decode, rs_kernels.hip).

    python tools/rs_bench.py [--steps 10] [--warmup 2] [--rows 8192] [--bytes 4460] [--nsym 32]

Workload: 8192 messages of 4460 bytes -- 20 full blocks of RS(255,223), 5100
encoded bytes -- with interleave 1 and 4; 64 distinct rows repeated over the
batch.  Cases: encode, decode of clean input, decode with 8 and with 16 random
errors in every block.  The GPU part runs in a child process of its own under
a time limit.  Timing: HIP events on the null stream around `steps` calls of
the device entry on device-resident input, after the warm-up calls.  Before
timing, the 64 distinct rows of every case -- bytes, out_len, corrected,
failed -- are checked against the numpy restatement (tests/rs_cases.py).

One JSON line: per case ms per call and GB/s of message bytes; for the clean
decode also `x_hbm`, the time over what its bytes (encoded in, message out)
would take at the 5.2 TB/s this project measured for HBM streams.
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

CHILD_LIMIT_S = 540
SAMPLE = 64
HBM_BPS = 5.2e12
INTERLEAVES = (1, 4)
ERRORS = (0, 8, 16)


def child(B: int, n_msg: int, nsym: int, steps: int, warmup: int) -> int:
    import _amr
    import rs_cases as rc
    _amr.require_gpu()
    lib = _amr.lib()
    _amr.check(lib.amr_set_device(_amr.default_device()))
    hip = ctypes.CDLL("libamdhip64.so")
    L = rc.encoded_len(n_msg, nsym)
    nblk = len(rc.block_lens(L))
    ns = min(SAMPLE, B)
    bufs = []

    def dmalloc(nbytes):
        p = ctypes.c_void_p()
        _amr.check(lib.amr_malloc(ctypes.byref(p), max(1, nbytes)))
        bufs.append(p)
        return p

    def hipcheck(rc_, what):
        if rc_ != 0:
            raise RuntimeError(f"{what}: hip error {rc_}")

    def tile(d_dst, rows, width):
        """The distinct rows repeated over the B device rows."""
        for r0 in range(0, B, ns):
            k = min(ns, B - r0)
            _amr.check(lib.amr_memcpy_h2d(ctypes.c_void_p(d_dst.value + r0 * width), _amr.ptr(rows), k * width))

    def timed(step):
        for _ in range(max(1, warmup)):
            step()
        _amr.check(lib.amr_device_synchronize())
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
        return ms.value / 1e3 / steps

    cases = []
    try:
        d_msg, d_cw, d_out = dmalloc(B * n_msg), dmalloc(B * L), dmalloc(B * n_msg)
        d_mlen, d_clen, d_oln = dmalloc(B * 8), dmalloc(B * 8), dmalloc(B * 8)
        d_cor, d_bad = dmalloc(B * 4), dmalloc(B * 4)
        mlen, clen = np.full(B, n_msg, np.int64), np.full(B, L, np.int64)
        _amr.check(lib.amr_memcpy_h2d(d_mlen, _amr.ptr(mlen), mlen.nbytes))
        _amr.check(lib.amr_memcpy_h2d(d_clen, _amr.ptr(clen), clen.nbytes))
        rng = np.random.default_rng(1)
        msgs = rng.integers(0, 256, (ns, n_msg), dtype=np.uint8)
        tile(d_msg, msgs, n_msg)
        for I in INTERLEAVES:
            def enc():
                _amr.check(lib.amr_rs_encode_device(None, d_msg, n_msg, d_mlen, B, nsym, I, d_cw, L, d_oln))

            dt = timed(enc)
            cw = np.zeros((B, L), np.uint8)
            _amr.check(lib.amr_memcpy_d2h(_amr.ptr(cw), d_cw, cw.nbytes))
            want = [rc.encode(msgs[i].tobytes(), nsym, I) for i in range(ns)]
            same = sum(int(cw[i].tobytes() == want[i]) for i in range(ns))
            assert same == ns and np.array_equal(cw[B - 1], cw[(B - 1) % ns]), \
                f"GPU encode differs from the restatement ({same} of {ns} equal)"
            cases.append({"case": "encode", "interleave": I, "ms_per_call": round(dt * 1e3, 3),
                          "msg_GBps": round(B * n_msg / dt / 1e9, 1), "parity_sample": f"{same}/{ns}"})
            for ne in ERRORS:
                rx = np.stack([np.frombuffer(rc.corrupt_blocks(rng, w, nsym, I, ne)[0], np.uint8) for w in want])
                tile(d_cw, rx, L)

                def dec():
                    _amr.check(lib.amr_rs_decode_device(None, d_cw, L, d_clen, None, B, nsym, I, d_out, n_msg, d_oln,
                                                        d_cor, d_bad))

                dt = timed(dec)
                out = np.zeros((B, n_msg), np.uint8)
                oln, cor, bad = np.zeros(B, np.int64), np.zeros(B, np.int32), np.zeros(B, np.int32)
                for dst, src in ((out, d_out), (oln, d_oln), (cor, d_cor), (bad, d_bad)):
                    _amr.check(lib.amr_memcpy_d2h(_amr.ptr(dst), src, dst.nbytes))
                ref = rc.decode_batch([rx[i].tobytes() for i in range(ns)], nsym, I)
                same = sum(int((out[i, :oln[i]].tobytes(), int(cor[i]), int(bad[i])) == ref[i]) for i in range(ns))
                good = sum(int(ref[i][0] == msgs[i].tobytes()) for i in range(ns))
                last = B - 1
                assert same == ns and np.array_equal(out[last], out[last % ns]) and cor[last] == cor[last % ns], \
                    f"GPU decode differs from the restatement ({same} of {ns} equal)"
                case = {"case": f"decode_{ne}_errors_per_block" if ne else "decode_clean", "interleave": I,
                        "ms_per_call": round(dt * 1e3, 3), "msg_GBps": round(B * n_msg / dt / 1e9, 1),
                        "parity_sample": f"{same}/{ns}", "sample_recovered": f"{good}/{ns}"}
                if ne == 0:
                    case["x_hbm"] = round(dt / (B * (L + n_msg) / HBM_BPS), 1)
                cases.append(case)
    finally:
        for p in bufs:
            lib.amr_free(p)
    print(json.dumps({"rows": B, "message_bytes": n_msg, "encoded_bytes": L, "blocks_per_row": nblk, "nsym": nsym,
                      "steps": steps, "cases": cases}), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rows", type=int, default=8192)
    ap.add_argument("--bytes", type=int, default=4460)
    ap.add_argument("--nsym", type=int, default=32)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.rows, a.bytes, a.nsym, a.steps, a.warmup)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--steps", str(a.steps), "--warmup",
                            str(a.warmup), "--rows", str(a.rows), "--bytes", str(a.bytes), "--nsym", str(a.nsym)],
                           timeout=CHILD_LIMIT_S)
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": f"time limit of {CHILD_LIMIT_S} s"}), flush=True)
        return 124                                          # nothing more is started on the GPU after a hang
    if r.returncode != 0:
        print(json.dumps({"error": f"exit status {r.returncode}"}), flush=True)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
