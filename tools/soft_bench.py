#!/usr/bin/env python3
"""Time the soft-input Viterbi decoder (k_viterbi_soft) beside the hard one
(k_viterbi), and the PSK soft stage (K4s, k_psk_soft).  DESIGN §3g.

    python tools/soft_bench.py [--steps 10] [--warmup 2] [--rounds 5] [--codewords 8192] [--bytes 4798]
                               [--streams 4096] [--samples 96000]

Decoders: 8192 codewords of 4798 bytes (2398 message bytes), 2 % of the coded
bits inverted, 256 distinct codewords repeated over the batch; the soft decoder
reads the same codewords in bit-stream form (16 n + 12 int8 values at +-64).
A round times `steps` calls of amr_viterbi_decode_device and then `steps`
calls of amr_viterbi_decode_soft_device between HIP events on the null stream,
on device-resident input; the rounds alternate the two, and the figures are
the medians over the rounds with their spread.  Before timing, a sample of the
soft decoder's output -- bytes and metrics -- is checked against the numpy
restatement (tests/soft_cases.py) and against the hard decoder's messages.

K4s: 4096 streams of 96000 samples, QPSK at 9600 baud, lane layout.  The soft
stage runs inside the plan's sync_pack timing slot, after K4a and k_sync_pack;
its time is that slot's time in a soft call minus the slot's time in a hard
call on the same plan and input, the calls alternated, medians over the rounds.

No pass/fail threshold.  The GPU part runs in a child process of its own under
a time limit.  One JSON line.
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
DISTINCT = 256
SAMPLE = 8
BER = 0.02
MAG = 64


def spread(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def decoders(B: int, L: int, steps: int, warmup: int, rounds: int) -> dict:
    import _amr
    import fec
    import soft_cases as sc
    import viterbi_cases as vc
    assert vc.is_codeword_len(L), "--bytes must be a codeword length (even, >= 2)"
    lib = _amr.lib()
    hip = ctypes.CDLL("libamdhip64.so")
    n_msg = (L - 2) // 2
    nv = 16 * n_msg + 12
    ocap = max(1, n_msg)
    cases = vc.noisy(1, [n_msg] * DISTINCT, BER)
    msgs = [m for m, _ in cases]
    hard_tile = np.stack([np.frombuffer(rx, np.uint8) for _, rx in cases])
    soft_tile = np.stack([fec.ViterbiDecoder.soft_from_bytes(rx, MAG) for _, rx in cases])
    wb_h = int(lib.amr_viterbi_work_bytes(L, B))
    wb_s = int(lib.amr_viterbi_soft_work_bytes(nv, B))
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
        d_h, d_s = dmalloc(B * L), dmalloc(B * nv)
        d_hl, d_sl, d_out = dmalloc(B * 8), dmalloc(B * 8), dmalloc(B * ocap)
        d_oln, d_met, d_work = dmalloc(B * 8), dmalloc(B * 4), dmalloc(max(wb_h, wb_s))
        for r0 in range(0, B, DISTINCT):
            k = min(DISTINCT, B - r0)
            _amr.check(lib.amr_memcpy_h2d(ctypes.c_void_p(d_h.value + r0 * L), _amr.ptr(hard_tile), k * L))
            _amr.check(lib.amr_memcpy_h2d(ctypes.c_void_p(d_s.value + r0 * nv), _amr.ptr(soft_tile), k * nv))
        hard_lens, soft_lens = np.full(B, L, np.int64), np.full(B, nv, np.int64)
        _amr.check(lib.amr_memcpy_h2d(d_hl, _amr.ptr(hard_lens), B * 8))
        _amr.check(lib.amr_memcpy_h2d(d_sl, _amr.ptr(soft_lens), B * 8))

        def hard():
            _amr.check(lib.amr_viterbi_decode_device(None, d_h, L, d_hl, B, d_out, ocap, d_oln, d_met, d_work, wb_h))

        def soft():
            _amr.check(lib.amr_viterbi_decode_soft_device(None, d_s, nv, 0, d_sl, B, d_out, ocap, d_oln, d_met, d_work,
                                                          wb_s))

        def fetch():
            _amr.check(lib.amr_device_synchronize())
            out, met, oln = np.zeros((B, ocap), np.uint8), np.zeros(B, np.int32), np.zeros(B, np.int64)
            _amr.check(lib.amr_memcpy_d2h(_amr.ptr(out), d_out, out.nbytes))
            _amr.check(lib.amr_memcpy_d2h(_amr.ptr(met), d_met, met.nbytes))
            _amr.check(lib.amr_memcpy_d2h(_amr.ptr(oln), d_oln, oln.nbytes))
            return [out[i, :oln[i]].tobytes() for i in range(B)], met

        for _ in range(max(1, warmup)):
            hard()
        h_out, h_met = fetch()
        for _ in range(max(1, warmup)):
            soft()
        s_out, s_met = fetch()
        ns = min(SAMPLE, B, DISTINCT)
        want = sc.soft_decode_batch([soft_tile[i] for i in range(ns)])
        same = sum(int(s_out[i] == want[i][0] and int(s_met[i]) == want[i][1]) for i in range(ns))
        assert same == ns, f"soft GPU decode differs from the restatement ({same} of {ns} equal)"
        # at one magnitude the soft metric is the hard one times it
        assert s_out == h_out and np.array_equal(s_met, h_met * MAG), "soft at one magnitude differs from hard"
        corrected = sum(int(s_out[i] == msgs[i]) for i in range(min(B, DISTINCT)))

        ev0, ev1 = ctypes.c_void_p(), ctypes.c_void_p()
        hipcheck(hip.hipEventCreate(ctypes.byref(ev0)), "hipEventCreate")
        hipcheck(hip.hipEventCreate(ctypes.byref(ev1)), "hipEventCreate")

        def window(fn):
            hipcheck(hip.hipEventRecord(ev0, None), "hipEventRecord")
            for _ in range(steps):
                fn()
            hipcheck(hip.hipEventRecord(ev1, None), "hipEventRecord")
            hipcheck(hip.hipEventSynchronize(ev1), "hipEventSynchronize")
            ms = ctypes.c_float()
            hipcheck(hip.hipEventElapsedTime(ctypes.byref(ms), ev0, ev1), "hipEventElapsedTime")
            return ms.value / steps

        th, ts = [], []
        for _ in range(rounds):
            th.append(window(hard))
            ts.append(window(soft))
        hip.hipEventDestroy(ev0)
        hip.hipEventDestroy(ev1)
    finally:
        for p in bufs:
            lib.amr_free(p)
    mh, ms_ = spread(th), spread(ts)
    T = 4 * L - 2
    return {"codewords": B, "coded_bytes": L, "message_bytes": n_msg, "soft_values": nv, "ber": BER,
            "steps": steps, "rounds": rounds, "hard_ms_per_call": mh, "soft_ms_per_call": ms_,
            "soft_over_hard": round(ms_["median"] / mh["median"], 3),
            "soft_trellis_Gsteps_per_s": round(B * T / ms_["median"] / 1e6, 3),
            "hard_trellis_Gsteps_per_s": round(B * T / mh["median"] / 1e6, 3),
            "soft_input_bytes_per_codeword": nv, "hard_input_bytes_per_codeword": L,
            "survivor_bytes_per_codeword": wb_s // B, "parity_sample": f"{same}/{ns}",
            "corrected": f"{corrected}/{min(B, DISTINCT)}"}


def soft_stage(B: int, n: int, rounds: int) -> dict:
    import _amr
    import synth
    baud = 9600
    x = synth.qpsk_batch(B, n, baud, seed=2, distinct=min(B, 64))
    pl = _amr.PskPlan("qpsk", n, baud, max_streams=B)
    pl.set_layout("lane")
    pl.enable_timing(True)
    hard_out, _ = pl.demod_host(x)                          # warm both shapes
    outs, _, softs = pl.demod_soft_host(x)
    assert outs == hard_out and all(np.packbits(s > 0).tobytes() == o for s, o in zip(softs[:64], outs[:64]))
    th, ts = [], []
    for _ in range(rounds):
        pl.demod_host(x)
        th.append(pl.timings()["sync_pack"])
        pl.demod_soft_host(x)
        ts.append(pl.timings()["sync_pack"])
    mh, ms_ = spread(th), spread(ts)
    vals = sum(s.size for s in softs)
    k4s = ms_["median"] - mh["median"]
    return {"streams": B, "samples": n, "baud": baud, "layout": "lane", "rounds": rounds,
            "sync_pack_slot_hard_ms": mh, "sync_pack_slot_soft_ms": ms_, "k4s_ms": round(k4s, 4),
            "soft_values": vals, "k4s_Gvalues_per_s": round(vals / k4s / 1e6, 2) if k4s > 0 else None}


def child(a) -> int:
    import _amr
    _amr.require_gpu()
    _amr.check(_amr.lib().amr_set_device(_amr.default_device()))
    res = {"decoder": decoders(a.codewords, a.bytes, a.steps, a.warmup, a.rounds),
           "k4s": soft_stage(a.streams, a.samples, a.rounds)}
    print(json.dumps(res), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--codewords", type=int, default=8192)
    ap.add_argument("--bytes", type=int, default=4798)
    ap.add_argument("--streams", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=96000)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] +
                           [f"--{k}={getattr(a, k)}" for k in ("steps", "warmup", "rounds", "codewords", "bytes",
                                                               "streams", "samples")], timeout=CHILD_LIMIT_S)
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": f"time limit of {CHILD_LIMIT_S} s"}), flush=True)
        return 124                                          # nothing more is started on the GPU after a hang
    if r.returncode != 0:
        print(json.dumps({"error": f"exit status {r.returncode}"}), flush=True)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
