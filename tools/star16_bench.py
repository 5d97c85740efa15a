#!/usr/bin/env python3
"""Time a star16 demodulation step beside the d8psk and QPSK steps on the same
input, and the star16 soft stage (k_psk_soft16).  DESIGN §3o.

    python tools/star16_bench.py [--streams 8192] [--samples 96000] [--steps 16] [--warmup 2] [--rounds 5]
                                 [--inflight 4]

Batches of 8192 float32 streams of 96000 samples at 9600 Bd on a 12 kHz
carrier: 64 distinct star16 frames from the GPU modulator, tiled over a batch
with N(0, 0.05^2) of its own per stream and batch (amr_synth_tile_noise),
resident on the device, `inflight` such batches.  `inflight` plans of each of
star16, d8psk and qpsk (each its own HIP stream and scratch, as bench.py keeps
them) demodulate those buffers through the device entry in the lane layout,
every plan told `inflight` batches are in flight (the QPSK low-pass then
slices fused, as the headline workload's does; star16 and d8psk plans never
fuse and slice in k_slice16 / k_slice8).  A window queues `steps` batches
round-robin over one kind's plans and waits for all of them, a host clock
around it; a round times the three kinds in turn, then one batch ALONE on one
plan of each kind, that plan told so; the figures are the medians over the
rounds with their spread, and the ratios of the medians.  --hw-queues (default
32, as bench.py) is the process's GPU_MAX_HW_QUEUES.

Before timing, the star16 bytes of a sample of streams are checked against the
numpy restatement (tests/star16_cases.py), and the payload bytes that differ
from what was sent are counted.  After it, with one plan's timing slots on per
kind: its slots for one call alone (sync_pack is the slicer + sync / pack
slot), and the soft stage's time as the sync_pack slot of a soft call minus
that of a hard call on the star16 plan, alternated, medians over the rounds.
The slot is also given as a multiple of the time the slicer's symbol reads
(16 B per symbol and stream) take at --stream-rate TB/s (default 5.2, the
streaming rate DESIGN §4 records): an upper bound of k_slice16's own multiple,
since the slot holds k_sync_pack too.

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
BAUD, CARRIER = 9600, 12000.0
KINDS = ("star16", "d8psk", "qpsk")
DISTINCT = 64
SAMPLE = 4
SIGMA = 0.05


def spread(v):
    v = sorted(v)
    return {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}


def child(a) -> int:
    import _amr
    import modem
    import star16_cases as s16
    _amr.require_gpu()
    lib = _amr.lib()
    _amr.check(lib.amr_set_device(_amr.default_device()))
    B, n = a.streams, a.samples
    sps = 96000 // BAUD
    rng = np.random.default_rng(16)
    room = max(1, (n // sps - 40) // 2 - 4)
    frames = [b"FB" + rng.integers(0, 256, room, dtype=np.uint8).tobytes() for _ in range(min(DISTINCT, B))]
    base = np.ascontiguousarray(modem.modulate_batch("star16", frames, BAUD, CARRIER, n_out=n))
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
        d_x = d_xs[0]
        io = {}
        for kind in KINDS:
            plans[kind] = []
            for k in range(P):
                pl = _amr.PskPlan(kind, n, BAUD, CARRIER, max_streams=B)
                pl.set_layout("lane")
                pl.set_inflight(P)
                plans[kind].append(pl)
                io[kind, k] = (dmalloc(B * pl.out_cap), dmalloc(B * 8), dmalloc(B * 8))

        def call(kind, k=0):
            pl = plans[kind][k]
            d_out, d_len, d_sync = io[kind, k]
            _amr.check(lib.amr_psk_demod_device(pl.handle, d_xs[k], _amr.DTYPE_F32, B, n, d_out, pl.out_cap, d_len,
                                                d_sync))

        def sync(kind, k=None):
            for pl in plans[kind] if k is None else [plans[kind][k]]:
                _amr.check(lib.amr_psk_plan_synchronize(pl.handle))

        for kind in plans:
            for _ in range(max(1, a.warmup)):
                for k in range(P):
                    call(kind, k)
            sync(kind)
        lowpass = {k: plans[k][0].last_lowpass() for k in plans}
        layouts = {k: plans[k][0].last_layout() for k in plans}
        # a sample of the star16 output against the restatement
        pl = plans["star16"][0]
        ns = min(SAMPLE, B)
        xs = np.zeros((ns, n), np.float32)
        out, ln = np.zeros((ns, pl.out_cap), np.uint8), np.zeros(ns, np.int64)
        _amr.check(lib.amr_memcpy_d2h(_amr.ptr(xs), d_x, xs.nbytes))
        _amr.check(lib.amr_memcpy_d2h(_amr.ptr(out), io["star16", 0][0], out.nbytes))
        _amr.check(lib.amr_memcpy_d2h(_amr.ptr(ln), io["star16", 0][1], ln.nbytes))
        same = sum(int(out[i, :ln[i]].tobytes() == s16.demod(xs[i], BAUD, CARRIER)[0]) for i in range(ns))
        assert same == ns, f"star16 GPU bytes differ from the restatement ({same} of {ns} equal)"
        # how the link itself does at this rate and noise: payload bytes that differ from what was sent
        sent = [np.frombuffer(frames[i], np.uint8) for i in range(ns)]
        wrong = sum(int(np.count_nonzero(out[i, :sent[i].size] != sent[i])) for i in range(ns))

        def window(kind, alone=False):
            _amr.check(lib.amr_device_synchronize())
            t0 = time.perf_counter()
            if alone:
                plans[kind][0].set_inflight(1)
                call(kind)
                sync(kind, 0)
                ms = (time.perf_counter() - t0) * 1e3
                alone_lowpass[kind] = plans[kind][0].last_lowpass()
                plans[kind][0].set_inflight(P)
                return ms
            for j in range(a.steps):
                call(kind, j % P)
            sync(kind)
            return (time.perf_counter() - t0) * 1e3 / a.steps

        tf, ta = {k: [] for k in KINDS}, {k: [] for k in KINDS}
        alone_lowpass = {}
        for kind in plans:                                  # the lone-batch shape once before it is timed
            window(kind, alone=True)
        for _ in range(a.rounds):
            for kind in KINDS:
                tf[kind].append(window(kind))
            for kind in KINDS:
                ta[kind].append(window(kind, alone=True))

        # the stages, and the soft stage: timing slots on (events around every stage), one plan alone
        slots = {}
        for kind in plans:
            plans[kind][0].enable_timing(True)
            plans[kind][0].set_inflight(1)
            call(kind)
            sync(kind, 0)
            slots[kind] = {k: round(v, 4) for k, v in plans[kind][0].timings().items()}
        stride = 8 * pl.out_cap
        d_soft = dmalloc(B * stride)
        d_out, d_len, d_sync = io["star16", 0]

        def soft_call():
            _amr.check(lib.amr_psk_demod_soft_device(pl.handle, d_x, _amr.DTYPE_F32, B, n, d_out, pl.out_cap, d_len,
                                                     d_sync, None, d_soft, stride))
        soft_call()
        sync("star16", 0)
        sv = np.zeros(min(stride, 4096), np.int8)
        _amr.check(lib.amr_memcpy_d2h(_amr.ptr(sv), d_soft, sv.nbytes))
        k = min(sv.size, 8 * int(ln[0])) // 8 * 8
        assert np.packbits(sv[:k] > 0).tobytes() == out[0, :k // 8].tobytes(), "soft signs are not the hard bits"
        th, ts = [], []
        for _ in range(a.rounds):
            call("star16")
            sync("star16", 0)
            th.append(pl.timings()["sync_pack"])
            soft_call()
            sync("star16", 0)
            ts.append(pl.timings()["sync_pack"])
    finally:
        plans.clear()
        for p in bufs:
            lib.amr_free(p)
    mf, ma = {k: spread(v) for k, v in tf.items()}, {k: spread(v) for k, v in ta.items()}
    mh, ms_ = spread(th), spread(ts)
    n_sym = (n - sps // 2 + sps - 1) // sps
    vals = B * 4 * (n_sym - 1)
    k16 = ms_["median"] - mh["median"]
    read_ms = B * n_sym * 16 / (a.stream_rate * 1e12) * 1e3     # the slicer's symbol reads at the streaming rate
    slot = slots["star16"]["sync_pack"]

    def ratio(x, y, m):
        return round(m[x]["median"] / m[y]["median"], 4)
    res = {"streams": B, "samples": n, "baud": BAUD, "carrier": CARRIER, "inflight": P, "steps": a.steps,
           "rounds": a.rounds, "layout": layouts, "lowpass": lowpass, "ms_per_step": mf, "alone_ms": ma,
           "star16_over_d8psk": ratio("star16", "d8psk", mf), "star16_over_qpsk": ratio("star16", "qpsk", mf),
           "star16_over_d8psk_alone": ratio("star16", "d8psk", ma),
           "star16_over_qpsk_alone": ratio("star16", "qpsk", ma), "lowpass_alone": alone_lowpass,
           "slots_alone_ms": slots, "hw_queues": int(os.environ.get("GPU_MAX_HW_QUEUES", "4")),
           "sync_pack_slot_hard_ms": mh, "sync_pack_slot_soft_ms": ms_, "soft16_ms": round(k16, 4),
           "soft_values": vals, "soft16_Gvalues_per_s": round(vals / k16 / 1e6, 2) if k16 > 0 else None,
           "symbol_read_ms_at_stream_rate": round(read_ms, 4), "stream_rate_TBps": a.stream_rate,
           "slice_sync_pack_slot_over_symbol_reads": round(slot / read_ms, 2),
           "parity_sample": f"{same}/{ns}", "payload_byte_errors": f"{wrong}/{sum(v.size for v in sent)}"}
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
    ap.add_argument("--stream-rate", type=float, default=5.2, help="TB/s the symbol reads are held against")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] +
                           [f"--{k}={getattr(a, k)}" for k in ("streams", "samples", "steps", "warmup", "rounds",
                                                               "inflight")] + [f"--stream-rate={a.stream_rate}"], timeout=CHILD_LIMIT_S,
                           env=dict(os.environ, GPU_MAX_HW_QUEUES=str(max(1, min(32, a.hw_queues)))))
    except subprocess.TimeoutExpired:
        print(json.dumps({"error": f"time limit of {CHILD_LIMIT_S} s"}), flush=True)
        return 124                                          # nothing more is started on the GPU after a hang
    if r.returncode != 0:
        print(json.dumps({"error": f"exit status {r.returncode}"}), flush=True)
    return r.returncode


if __name__ == "__main__":
    sys.exit(main())
