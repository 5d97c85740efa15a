#!/usr/bin/env python3
"""Time an ofdm demodulation step beside the QPSK step (what the
ofdm_demodulate_simple alias costs) on the same input.  DESIGN §3j.

    python tools/ofdm_bench.py [--streams 8192] [--samples 96000] [--steps 16] [--warmup 2] [--rounds 5]
                               [--inflight 4] [--acquire [--window-streams 256]]

Batches of 8192 float32 streams of 96000 samples at 9600 Bd on a 12 kHz
carrier, 8 subcarriers (BASELINE configs[3]'s input shape): 64 distinct ofdm
frames from the GPU modulator, tiled over a batch with N(0, 0.05^2) of its own
per stream and batch (amr_synth_tile_noise), resident on the device, `inflight`
such batches.  `inflight` ofdm plans and as many qpsk plans (each its own HIP
stream and scratch, as bench.py keeps them; the qpsk plans in the lane layout,
told `inflight` batches are in flight) demodulate those buffers through the
device entry.  A window queues `steps` batches round-robin over one kind's
plans and waits for all of them, a host clock around it; a round times the
qpsk plans, then the ofdm plans, then one batch ALONE on one plan of each
kind; the figures are the medians over the rounds with their spread, and the
ratios of the medians.  Then, with one ofdm plan's timing slots on, its slots
for one call alone, medians over the rounds.

By arithmetic from the shapes: the bytes the ofdm step must move (x read once,
Y written by the DFT and read by the slicer, the words and bytes) as a share of
the 5.2 TB/s streaming rate DESIGN §4 records, and its FP64 operations (2
products and 2 sums per sample, subcarrier and useful sample; no fma) as a
share of the 78.6 TFLOP/s vector FP64 peak (which counts an fma as two, so a
kernel of separate products and sums tops out at half of it).

In every run, the ofdm bytes of a sample of streams are checked against the
numpy restatement (tests/ofdm_cases.py) before timing.

--acquire times acquisition instead, on the same shape: every
distinct frame is delayed by a seeded t < L before it is tiled, so no stream
starts on a symbol boundary.  The same plans run, through their device entries,
the unacquired demodulation, the acquisition alone (amr_ofdm_acquire_device)
and acquisition + demodulation (amr_ofdm_demod_acq_device): one batch alone and
`inflight` in flight, medians over the rounds with their spread; then the
timing slots of one acquired call alone.  By arithmetic: the fold reads x once,
its time at the 5.2 TB/s streaming rate, and the measured multiple of it beside
the DFT slot's own multiple.  Then the acquire slot at the largest symbol
(K = 64 at 1200 Bd: L = 5120, L * Ncp = 3.3 M additions of the window sum per
stream) on --window-streams streams.  Before timing, a sample of streams is
checked against the numpy restatement (tests/ofdm_acquire_cases.py): offsets
and bytes.

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
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "audio-modem-radio_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

CHILD_LIMIT_S = 540
BAUD, CARRIER, K = 9600, 12000.0, 8
DISTINCT = 64
SAMPLE = 4
SIGMA = 0.05
HBM_STREAM_BPS = 5.2e12
FP64_PEAK = 78.6e12


def spread(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def child(a) -> int:
    import _amr
    import modem
    import ofdm_cases as oc
    _amr.require_gpu()
    lib = _amr.lib()
    _amr.check(lib.amr_set_device(_amr.default_device()))
    B, n = a.streams, a.samples
    sps, L, Ncp, Nu, _ = oc.geometry(BAUD, CARRIER, K)
    S = n // L
    rng = np.random.default_rng(23)
    room = max(1, (2 * K * (S - 1) - 80) // 8 - 2)
    frames = [b"FB" + rng.integers(0, 256, room, dtype=np.uint8).tobytes() for _ in range(min(DISTINCT, B))]
    base = np.ascontiguousarray(modem.modulate_batch("ofdm", frames, BAUD, CARRIER, n_out=n, num_subcarriers=K))
    bufs = []

    def dmalloc(nbytes):
        p = ctypes.c_void_p()
        _amr.check(lib.amr_malloc(ctypes.byref(p), max(1, int(nbytes))))
        bufs.append(p)
        return p

    P = max(1, a.inflight)
    plans = {}
    try:
        d_base = dmalloc(base.nbytes)
        _amr.check(lib.amr_memcpy_h2d(d_base, _amr.ptr(base), base.nbytes))
        d_xs = [dmalloc(B * n * 4) for _ in range(P)]
        for k, d in enumerate(d_xs):
            _amr.check(lib.amr_synth_tile_noise(d_base, base.shape[0], n, d, B, 17 * k, SIGMA, 7 + k))
        io = {}
        for kind in ("qpsk", "ofdm"):
            plans[kind] = []
            for k in range(P):
                if kind == "qpsk":
                    pl = _amr.PskPlan("qpsk", n, BAUD, CARRIER, max_streams=B)
                    pl.set_layout("lane")
                    pl.set_inflight(P)
                else:
                    pl = _amr.OfdmPlan(n, BAUD, CARRIER, K, max_streams=B)
                plans[kind].append(pl)
                io[kind, k] = (dmalloc(B * pl.out_cap), dmalloc(B * 8), dmalloc(B * 8))
        entry = {"qpsk": lib.amr_psk_demod_device, "ofdm": lib.amr_ofdm_demod_device}
        waiter = {"qpsk": lib.amr_psk_plan_synchronize, "ofdm": lib.amr_ofdm_plan_synchronize}

        def call(kind, k=0):
            pl = plans[kind][k]
            d_out, d_len, d_sync = io[kind, k]
            _amr.check(entry[kind](pl.handle, d_xs[k], _amr.DTYPE_F32, B, n, d_out, pl.out_cap, d_len, d_sync))

        def sync(kind, k=None):
            for pl in plans[kind] if k is None else [plans[kind][k]]:
                _amr.check(waiter[kind](pl.handle))

        for kind in plans:
            for _ in range(max(1, a.warmup)):
                for k in range(P):
                    call(kind, k)
            sync(kind)
        # a sample of the ofdm output against the restatement, and against what was sent
        pl = plans["ofdm"][0]
        ns = min(SAMPLE, B)
        xs = np.zeros((ns, n), np.float32)
        out, ln = np.zeros((ns, pl.out_cap), np.uint8), np.zeros(ns, np.int64)
        _amr.check(lib.amr_memcpy_d2h(_amr.ptr(xs), d_xs[0], xs.nbytes))
        _amr.check(lib.amr_memcpy_d2h(_amr.ptr(out), io["ofdm", 0][0], out.nbytes))
        _amr.check(lib.amr_memcpy_d2h(_amr.ptr(ln), io["ofdm", 0][1], ln.nbytes))
        same = sum(int(out[i, :ln[i]].tobytes() == oc.demod(xs[i], BAUD, CARRIER, K)[0]) for i in range(ns))
        assert same == ns, f"ofdm GPU bytes differ from the restatement ({same} of {ns} equal)"
        sent = [np.frombuffer(frames[i % len(frames)], np.uint8) for i in range(ns)]
        wrong = sum(int(np.count_nonzero(out[i, :sent[i].size] != sent[i])) for i in range(ns))

        def window(kind, alone=False):
            _amr.check(lib.amr_device_synchronize())
            t0 = time.perf_counter()
            if alone:
                call(kind)
                sync(kind, 0)
                return (time.perf_counter() - t0) * 1e3
            for j in range(a.steps):
                call(kind, j % P)
            sync(kind)
            return (time.perf_counter() - t0) * 1e3 / a.steps

        tq, to, aq, ao = [], [], [], []
        for _ in range(a.rounds):
            tq.append(window("qpsk"))
            to.append(window("ofdm"))
            aq.append(window("qpsk", alone=True))
            ao.append(window("ofdm", alone=True))
        pl.enable_timing(True)
        slot_runs = []
        for _ in range(a.rounds):
            call("ofdm")
            sync("ofdm", 0)
            slot_runs.append(pl.timings())
        slots = {k: spread([r[k] for r in slot_runs]) for k in slot_runs[0]}
    finally:
        plans.clear()
        for p in bufs:
            lib.amr_free(p)
    mq, mo, maq, mao = spread(tq), spread(to), spread(aq), spread(ao)
    n_bits = 2 * K * (S - 1)
    moved = B * (n * 4 + 2 * S * K * 16 + 2 * ((n_bits + 31) // 32) * 4 + n_bits // 8)
    flops = B * S * K * Nu * 4
    step_s, dft_s = mo["median"] * 1e-3, slots["dft"]["median"] * 1e-3
    res = {"streams": B, "samples": n, "baud": BAUD, "carrier": CARRIER, "subcarriers": K, "symbols": S, "Nu": Nu,
           "inflight": P, "steps": a.steps, "rounds": a.rounds, "qpsk_ms_per_step": mq, "ofdm_ms_per_step": mo,
           "qpsk_over_ofdm": round(mq["median"] / mo["median"], 3), "qpsk_alone_ms": maq, "ofdm_alone_ms": mao,
           "qpsk_over_ofdm_alone": round(maq["median"] / mao["median"], 3), "ofdm_slots_alone_ms": slots,
           "bytes_moved": moved, "share_of_5.2TBps_step": round(moved / step_s / HBM_STREAM_BPS, 4),
           "share_of_5.2TBps_dft_slot": round(B * (n * 4 + S * K * 16) / dft_s / HBM_STREAM_BPS, 4),
           "fp64_ops": flops, "share_of_fp64_peak_step": round(flops / step_s / FP64_PEAK, 4),
           "share_of_fp64_peak_dft_slot": round(flops / dft_s / FP64_PEAK, 4),
           "hw_queues": int(os.environ.get("GPU_MAX_HW_QUEUES", "4")), "parity_sample": f"{same}/{ns}",
           "payload_byte_errors": f"{wrong}/{sum(v.size for v in sent)}"}
    print(json.dumps(res), flush=True)
    return 0


def child_acquire(a) -> int:
    import _amr
    import modem
    import ofdm_acquire_cases as ac
    import ofdm_cases as oc
    _amr.require_gpu()
    lib = _amr.lib()
    _amr.check(lib.amr_set_device(_amr.default_device()))
    B, n = a.streams, a.samples
    sps, L, Ncp, Nu, _ = oc.geometry(BAUD, CARRIER, K)
    S = n // L
    rng = np.random.default_rng(23)
    room = max(1, (2 * K * (S - 2) - 80) // 8 - 2)          # a symbol less than the capture holds: room for the delay
    frames = [b"FB" + rng.integers(0, 256, room, dtype=np.uint8).tobytes() for _ in range(min(DISTINCT, B))]
    clean = modem.modulate_batch("ofdm", frames, BAUD, CARRIER, n_out=n, num_subcarriers=K)
    delays = rng.integers(1, L, len(frames))
    base = np.zeros_like(clean)
    for i, t in enumerate(delays):
        base[i, t:] = clean[i, :n - t]
    bufs = []

    def dmalloc(nbytes):
        p = ctypes.c_void_p()
        _amr.check(lib.amr_malloc(ctypes.byref(p), max(1, int(nbytes))))
        bufs.append(p)
        return p

    P = max(1, a.inflight)
    plans = []
    try:
        d_base = dmalloc(base.nbytes)
        _amr.check(lib.amr_memcpy_h2d(d_base, _amr.ptr(base), base.nbytes))
        d_xs = [dmalloc(B * n * 4) for _ in range(P)]
        for k, d in enumerate(d_xs):
            _amr.check(lib.amr_synth_tile_noise(d_base, base.shape[0], n, d, B, 17 * k, SIGMA, 7 + k))
        io = []
        for k in range(P):
            pl = _amr.OfdmPlan(n, BAUD, CARRIER, K, max_streams=B)
            plans.append(pl)
            io.append((dmalloc(B * pl.out_cap), dmalloc(B * 8), dmalloc(B * 8), dmalloc(B * 8)))

        def call(kind, k=0):
            pl = plans[k]
            d_out, d_len, d_sync, d_off = io[k]
            if kind == "ofdm":
                rc = lib.amr_ofdm_demod_device(pl.handle, d_xs[k], _amr.DTYPE_F32, B, n, d_out, pl.out_cap, d_len, d_sync)
            elif kind == "acquire":
                rc = lib.amr_ofdm_acquire_device(pl.handle, d_xs[k], _amr.DTYPE_F32, B, n, d_off, None, None)
            else:
                rc = lib.amr_ofdm_demod_acq_device(pl.handle, d_xs[k], _amr.DTYPE_F32, B, n, d_out, pl.out_cap, d_len,
                                                   d_sync, None, 0, d_off)
            _amr.check(rc)

        def sync(k=None):
            for pl in plans if k is None else [plans[k]]:
                pl.synchronize()

        kinds = ("ofdm", "acquire", "acq_demod")
        for kind in kinds:
            for _ in range(max(1, a.warmup)):
                for k in range(P):
                    call(kind, k)
            sync()
        # a sample of streams against the restatement (the last warm-up call was acq_demod), and against what was sent
        ns = min(SAMPLE, B)
        xs = np.zeros((ns, n), np.float32)
        out, ln, off = np.zeros((ns, plans[0].out_cap), np.uint8), np.zeros(ns, np.int64), np.zeros(ns, np.int64)
        _amr.check(lib.amr_memcpy_d2h(_amr.ptr(xs), d_xs[0], xs.nbytes))
        _amr.check(lib.amr_memcpy_d2h(_amr.ptr(out), io[0][0], out.nbytes))
        _amr.check(lib.amr_memcpy_d2h(_amr.ptr(ln), io[0][1], ln.nbytes))
        _amr.check(lib.amr_memcpy_d2h(_amr.ptr(off), io[0][3], off.nbytes))
        want = [ac.demod(xs[i], BAUD, CARRIER, K) for i in range(ns)]
        same = sum(int(out[i, :ln[i]].tobytes() == want[i][0] and off[i] == want[i][2]) for i in range(ns))
        assert same == ns, f"acquired GPU bytes / offsets differ from the restatement ({same} of {ns} equal)"
        exact = sum(int((off[i] + Ncp // 2 - delays[i % len(frames)]) % L == 0) for i in range(ns))
        sent = [np.frombuffer(frames[i % len(frames)], np.uint8) for i in range(ns)]
        wrong = sum(int(np.count_nonzero(out[i, :sent[i].size] != sent[i])) for i in range(ns))

        def window(kind, alone=False):
            _amr.check(lib.amr_device_synchronize())
            t0 = time.perf_counter()
            if alone:
                call(kind)
                sync(0)
                return (time.perf_counter() - t0) * 1e3
            for j in range(a.steps):
                call(kind, j % P)
            sync()
            return (time.perf_counter() - t0) * 1e3 / a.steps

        flight = {k: [] for k in kinds}
        alone = {k: [] for k in kinds}
        for _ in range(a.rounds):
            for kind in kinds:
                flight[kind].append(window(kind))
            for kind in kinds:
                alone[kind].append(window(kind, alone=True))
        pl = plans[0]
        pl.enable_timing(True)
        slot_runs = []
        for _ in range(a.rounds):
            call("acq_demod")
            sync(0)
            slot_runs.append(pl.timings())
        pl.enable_timing(False)
        slots = {k: spread([r[k] for r in slot_runs]) for k in slot_runs[0]}
        plans.clear()
        # the window sum at the largest symbol: K = 64 at 1200 Bd, the acquire slot of a call alone
        wK, wbaud, wcar, wB = 64, 1200, 3000.0, max(1, a.window_streams)
        _, wL, wNcp, wNu, _ = oc.geometry(wbaud, wcar, wK)
        wpl = _amr.OfdmPlan(n, wbaud, wcar, wK, max_streams=wB)
        plans.append(wpl)
        d_woff = dmalloc(wB * 8)
        wpl.enable_timing(True)
        wruns = []
        for _ in range(a.rounds + 1):
            _amr.check(lib.amr_ofdm_acquire_device(wpl.handle, d_xs[0], _amr.DTYPE_F32, min(wB, B), n, d_woff, None, None))
            wpl.synchronize()
            wruns.append(wpl.timings()["acquire"])
        wslot = spread(wruns[1:])
    finally:
        plans.clear()
        for p in bufs:
            lib.amr_free(p)
    fold_bytes = B * n * 4
    bound_ms = fold_bytes / HBM_STREAM_BPS * 1e3
    dft_bound_ms = B * (n * 4 + S * K * 16) / HBM_STREAM_BPS * 1e3
    wn = min(wB, B)
    res = {"mode": "acquire", "streams": B, "samples": n, "baud": BAUD, "carrier": CARRIER, "subcarriers": K, "L": L,
           "Ncp": Ncp, "inflight": P, "steps": a.steps, "rounds": a.rounds,
           "alone_ms": {k: spread(v) for k, v in alone.items()},
           "inflight_ms_per_step": {k: spread(v) for k, v in flight.items()},
           "acq_demod_slots_alone_ms": slots,
           "fold_bytes": fold_bytes, "fold_bound_ms_at_5.2TBps": round(bound_ms, 4),
           "acquire_slot_over_fold_bound": round(slots["acquire"]["median"] / bound_ms, 3),
           "acquire_alone_over_fold_bound": round(spread(alone["acquire"])["median"] / bound_ms, 3),
           "dft_slot_over_its_bound": round(slots["dft"]["median"] / dft_bound_ms, 3),
           "window_sum_case": {"subcarriers": wK, "baud": wbaud, "L": wL, "Ncp": wNcp, "streams": wn,
                               "periods": (n - wNu) // wL, "window_adds_per_stream": wL * wNcp,
                               "acquire_slot_ms": wslot,
                               "window_adds_per_s": round(wn * wL * wNcp / (wslot["median"] * 1e-3), 0)},
           "hw_queues": int(os.environ.get("GPU_MAX_HW_QUEUES", "4")), "parity_sample": f"{same}/{ns}",
           "timing_exact_sample": f"{exact}/{ns}", "payload_byte_errors": f"{wrong}/{sum(v.size for v in sent)}"}
    print(json.dumps(res), flush=True)
    return 0


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--streams", type=int, default=8192)
    ap.add_argument("--samples", type=int, default=96000)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--inflight", type=int, default=4)
    ap.add_argument("--hw-queues", type=int, default=32, help="GPU_MAX_HW_QUEUES for the GPU process (<= 32)")
    ap.add_argument("--acquire", action="store_true", help="time acquisition (DESIGN §3k) instead of the qpsk comparison")
    ap.add_argument("--window-streams", type=int, default=256, help="--acquire: streams of the K = 64, 1200 Bd case")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child_acquire(a) if a.acquire else child(a)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] +
                           [f"--{k}={getattr(a, k)}" for k in ("streams", "samples", "steps", "warmup", "rounds",
                                                               "inflight")] +
                           ([f"--window-streams={a.window_streams}", "--acquire"] if a.acquire else []),
                           timeout=CHILD_LIMIT_S,
                           env=dict(os.environ, GPU_MAX_HW_QUEUES=str(max(1, min(32, a.hw_queues)))))
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": f"time limit of {CHILD_LIMIT_S} s"}), flush=True)
        return 124                                          # nothing more is started on the GPU after a hang
    if r.returncode != 0:
        print(json.dumps({"error": f"exit status {r.returncode}"}), flush=True)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
