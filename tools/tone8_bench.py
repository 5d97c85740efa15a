#!/usr/bin/env python3
"""Time tone8's acquisition, symbol stage and acquired demodulation beside the
FSK step at 50 Bd on tones c and c + 50 (what the receiver of the ft8 alias's
output costs, the only yardstick there is) on the same buffers.  DESIGN §3n.

    python tools/tone8_bench.py [--streams 8192] [--samples 96000] [--steps 16] [--warmup 2] [--rounds 5]
                                [--inflight 4] [--search 3]

Batches of 8192 float32 streams of 96000 samples at 1200 Bd on a 3000 Hz
carrier (L = 80, c2 = 5, which admits a search of at most 3): 64 distinct
seeded frames from the GPU modulator, each from a sender a seeded number of
half tone spacings off the receiver and delayed by a seeded t < 5 L, tiled
over a batch with N(0, 1.0^2) of its own per stream and batch
(amr_synth_tile_noise; 1.0 is the level tests/test_tone8_host.py's ladder
cleared at this configuration), resident on the device, `inflight` such
batches.  `inflight` tone8 plans (each its own HIP stream and scratch) and as
many fsk plans as 150 GB hold work on those buffers through the device entries,
in one process.  A window queues `steps` batches round-robin over one kind's
plans and waits for all of them, a host clock around it; a round times the fsk
step, the acquisition alone (amr_tone8_acquire_device), the unacquired
demodulation (amr_tone8_demod_device, acquire = 0) and the acquired call
(acquire = 1), first in flight, then one batch ALONE on one plan; the figures
are the medians over the rounds with their spread.  Then the timing slots of
one acquired call alone.

By arithmetic from the shapes: the acquire slot against the FP64 issue bound of
k_tone8_acq -- 4 NB (1 + 55 / C) multiplies and adds per sample, no fma, at
256 CUs x 64 lanes x 2.4 GHz = 39.3 T per second -- and against its one read of
x at the 5.2 TB/s streaming rate DESIGN §4 records; the despread slot
(k_tone8_dft) against one read of x plus the Y write (128 B per symbol) at that
rate, and against its own 32 FP64 operations per sample.

In every run a sample of streams is checked against the numpy restatement
(tests/tone8_cases.py) before timing: starts, shifts and bytes.

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
BAUD, CARRIER = 1200, 3000.0
FSK_BAUD = 50
DISTINCT = 64
SAMPLE = 4
SIGMA = 1.0
HBM_STREAM_BPS = 5.2e12
FP64_OPS = 256 * 64 * 2.4e9                                  # one multiply or add per lane per clock
FSK_BUDGET = 150e9
KINDS = ("fsk", "acquire", "plain", "acq_demod")


def spread(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def child(a) -> int:
    import _amr
    import _fsk
    import modem
    import tone8_cases as tc
    _amr.require_gpu()
    lib = _amr.lib()
    _amr.check(lib.amr_set_device(_amr.default_device()))
    B, n, G = a.streams, a.samples, a.search
    L, T, c2, G = tc.geometry(BAUD, CARRIER, 96000, G)
    S = n // L
    C, NB = _amr.tone8_chunk(G), 15 + 2 * G
    rng = np.random.default_rng(23)
    room = max(1, (3 * (S - 7 - 6)) // 8 - 2)                # a bit less than the capture holds: room for the delay
    frames = [b"FB" + rng.integers(0, 256, room, dtype=np.uint8).tobytes() for _ in range(min(DISTINCT, B))]
    delays = rng.integers(0, 5 * L, len(frames))
    offs = rng.integers(-G, G + 1, len(frames))
    base = np.zeros((len(frames), n), np.float32)
    for i, (t, o) in enumerate(zip(delays, offs)):           # one modulator call per sender carrier
        w = modem.modulate_batch("tone8", [frames[i]], BAUD, CARRIER + int(o) * BAUD / 2, n_out=n)[0]
        base[i, t:] = w[:n - t]
    bufs = []

    def dmalloc(nbytes):
        p = ctypes.c_void_p()
        _amr.check(lib.amr_malloc(ctypes.byref(p), max(1, int(nbytes))))
        bufs.append(p)
        return p

    P = max(1, a.inflight)
    fsk_each = max(1, int(lib.amr_fsk_plan_bytes_estimate(n, 96000 // FSK_BAUD, 7, B)))
    PF = max(1, min(P, int(FSK_BUDGET // fsk_each)))
    plans = {"fsk": [], "tone8": []}
    try:
        d_base = dmalloc(base.nbytes)
        _amr.check(lib.amr_memcpy_h2d(d_base, _amr.ptr(base), base.nbytes))
        d_xs = [dmalloc(B * n * 4) for _ in range(P)]
        for k, d in enumerate(d_xs):
            _amr.check(lib.amr_synth_tile_noise(d_base, base.shape[0], n, d, B, 17 * k, SIGMA, 7 + k))
        io = {}
        for k in range(P):
            pt = _amr.Tone8Plan(n, BAUD, CARRIER, 96000, G, max_streams=B)
            plans["tone8"].append(pt)
            io["tone8", k] = (dmalloc(B * pt.out_cap), dmalloc(B * 8), dmalloc(B * 8), dmalloc(B * 8), dmalloc(B * 8))
        for k in range(PF):
            pf = _fsk.FskPlan(n, FSK_BAUD, CARRIER, CARRIER + FSK_BAUD, max_streams=B)
            plans["fsk"].append(pf)
            io["fsk", k] = (dmalloc(B * pf.out_cap), dmalloc(B * 8), dmalloc(B * 8))

        def count(kind):
            return PF if kind == "fsk" else P

        def call(kind, k=0):
            if kind == "fsk":
                pl = plans["fsk"][k]
                d_out, d_len, d_sync = io["fsk", k]
                rc = lib.amr_fsk_demod_device(pl.handle, d_xs[k], _amr.DTYPE_F32, B, n, d_out, pl.out_cap, d_len, d_sync)
            else:
                pl = plans["tone8"][k]
                d_out, d_len, d_sync, d_st, d_sh = io["tone8", k]
                if kind == "acquire":
                    rc = lib.amr_tone8_acquire_device(pl.handle, d_xs[k], _amr.DTYPE_F32, B, n, d_st, d_sh, None)
                else:
                    rc = lib.amr_tone8_demod_device(pl.handle, d_xs[k], _amr.DTYPE_F32, B, n, d_out, pl.out_cap, d_len,
                                                    d_sync, None, 0, d_st, d_sh, 1 if kind == "acq_demod" else 0)
            _amr.check(rc)

        def sync(kind, k=None):
            ps = plans["fsk" if kind == "fsk" else "tone8"]
            for pl in ps if k is None else [ps[k]]:
                _amr.check((lib.amr_fsk_plan_synchronize if kind == "fsk" else lib.amr_tone8_plan_synchronize)(pl.handle))

        for kind in KINDS:                                   # acq_demod last: its outputs are what the sample reads
            for _ in range(max(1, a.warmup)):
                for k in range(count(kind)):
                    call(kind, k)
            sync(kind)
        ns = min(SAMPLE, B)
        pl = plans["tone8"][0]
        xs = np.zeros((ns, n), np.float32)
        out, ln = np.zeros((ns, pl.out_cap), np.uint8), np.zeros(ns, np.int64)
        st, sh = np.zeros(ns, np.int64), np.zeros(ns, np.int64)
        _amr.check(lib.amr_memcpy_d2h(_amr.ptr(xs), d_xs[0], xs.nbytes))
        _amr.check(lib.amr_memcpy_d2h(_amr.ptr(out), io["tone8", 0][0], out.nbytes))
        _amr.check(lib.amr_memcpy_d2h(_amr.ptr(ln), io["tone8", 0][1], ln.nbytes))
        _amr.check(lib.amr_memcpy_d2h(_amr.ptr(st), io["tone8", 0][3], st.nbytes))
        _amr.check(lib.amr_memcpy_d2h(_amr.ptr(sh), io["tone8", 0][4], sh.nbytes))
        want = [tc.demod(xs[i], BAUD, CARRIER, 96000, True, G) for i in range(ns)]
        same = sum(int(out[i, :ln[i]].tobytes() == want[i][0] and (st[i], sh[i]) == want[i][2:]) for i in range(ns))
        assert same == ns, f"acquired GPU bytes / starts / shifts differ from the restatement ({same} of {ns} equal)"
        found = sum(int(abs(st[i] - delays[i % len(frames)]) <= T and sh[i] == offs[i % len(frames)]) for i in range(ns))
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
                call(kind, j % count(kind))
            sync(kind)
            return (time.perf_counter() - t0) * 1e3 / a.steps

        flight = {k: [] for k in KINDS}
        alone = {k: [] for k in KINDS}
        for _ in range(a.rounds):
            for kind in KINDS:
                flight[kind].append(window(kind))
            for kind in KINDS:
                alone[kind].append(window(kind, alone=True))
        pl.enable_timing(True)
        slot_runs = []
        for _ in range(a.rounds):
            call("acq_demod")
            sync("acq_demod", 0)
            slot_runs.append(pl.timings())
        pl.enable_timing(False)
        slots = {k: spread([r[k] for r in slot_runs]) for k in slot_runs[0]}
    finally:
        plans.clear()
        for p in bufs:
            lib.amr_free(p)
    hbm_ms = B * n * 4 / HBM_STREAM_BPS * 1e3
    acq_ops = B * n * 4 * NB * (1 + 55 / C)
    acq_fp64_ms = acq_ops / FP64_OPS * 1e3
    dft_hbm_ms = B * (n * 4 + S * 128) / HBM_STREAM_BPS * 1e3
    dft_fp64_ms = B * n * 32 / FP64_OPS * 1e3
    res = {"streams": B, "samples": n, "baud": BAUD, "carrier": CARRIER, "L": L, "c2": c2, "search": G, "lines": NB,
           "chunk": C, "sigma": SIGMA, "inflight": P, "fsk_plans": PF, "fsk_baud": FSK_BAUD, "steps": a.steps,
           "rounds": a.rounds,
           "alone_ms": {k: spread(v) for k, v in alone.items()},
           "inflight_ms_per_step": {k: spread(v) for k, v in flight.items()},
           "acq_demod_slots_alone_ms": slots,
           "x_read_ms_at_5.2TBps": round(hbm_ms, 4),
           "acq_fp64_ops": int(acq_ops), "acq_fp64_bound_ms_at_39.3Tops": round(acq_fp64_ms, 4),
           "acquire_slot_over_fp64_bound": round(slots["acquire"]["median"] / acq_fp64_ms, 3),
           "acquire_slot_over_x_read": round(slots["acquire"]["median"] / hbm_ms, 3),
           "dft_hbm_bound_ms_at_5.2TBps": round(dft_hbm_ms, 4), "dft_fp64_bound_ms_at_39.3Tops": round(dft_fp64_ms, 4),
           "despread_slot_over_its_hbm_bound": round(slots["despread"]["median"] / dft_hbm_ms, 3),
           "despread_slot_over_its_fp64_bound": round(slots["despread"]["median"] / dft_fp64_ms, 3),
           "acq_demod_over_fsk_alone": round(spread(alone["acq_demod"])["median"] / spread(alone["fsk"])["median"], 4),
           "acq_demod_over_fsk_inflight": round(spread(flight["acq_demod"])["median"] / spread(flight["fsk"])["median"], 4),
           "hw_queues": int(os.environ.get("GPU_MAX_HW_QUEUES", "4")), "parity_sample": f"{same}/{ns}",
           "found_sample": f"{found}/{ns}", "payload_byte_errors": f"{wrong}/{sum(v.size for v in sent)}"}
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
    ap.add_argument("--search", type=int, default=3, help="half tone spacings searched either way (<= 3 on 3000 Hz)")
    ap.add_argument("--hw-queues", type=int, default=32, help="GPU_MAX_HW_QUEUES for the GPU process (<= 32)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] +
                           [f"--{k}={getattr(a, k)}" for k in ("streams", "samples", "steps", "warmup", "rounds",
                                                               "inflight", "search")],
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
