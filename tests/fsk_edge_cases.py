"""FSK captures at the edges of fsk_demodulate's parameter space (the
reference's modem.py:298-341 accepts all of them): the case list of
tests/golden/make_fsk_edge_golden.py and the seeded generator of its inputs.

Classes (params.edge in tests/golden/fsk_edge_manifest.json):
  lowbaud   a narrow band-pass: 45.45 (a float) .. 110 Bd at RTTY tones, 300 Bd
            at 8 / 11.025 / 22.05 kHz, 1200 Bd at 192 kHz
  edge0     (mark - baud) / nyq = 1e-6, 1e-3, and exactly 0 (scipy raises)
  edgenyq   (space + baud) / nyq = 1 - 1e-6, 1 - 1e-3, and exactly 1 (raises)
  same      mark == space: every compare a tie of two equal envelopes
  overlap   space = mark + baud: the tone bands overlap by half
  swapped   mark > space
  slow      baud / samp_rate < ~7e-6: the band-pass's impulse response has not
            decayed below 1e-40 within the 4 000 000 steps the library walks
            (csrc/iir_design.h), so it finds no FFT rounding bound
  unstable  low tones at low baud: butter(3, band)'s six-pole transfer-function
            form has a pole outside the unit circle by coefficient rounding;
            the reference decides its bytes from inf / NaN envelopes

Most inputs are too long to commit, so every input is regenerated from its
seed (make_input) and checked against the SHA-256 the manifest recorded when
the reference ran; the short ones are also stored (fsk_edge.npz).  Samples sit
on the 2^-15 grid (floats) or are int16, so a last-ulp difference in a host's
sin / normal does not move them."""
from __future__ import annotations

import hashlib

import numpy as np

STORE_BYTES = 48 * 1024          # inputs up to this size are also stored in fsk_edge.npz


def _c(edge, baud, f0, f1, fs, n, dtype, seed, kind="frame", noise=0.05, level=1.0):
    return dict(edge=edge, baud=baud, f0=float(f0), f1=float(f1), samp_rate=float(fs), n=int(n), dtype=dtype,
                seed=int(seed), kind=kind, noise=float(noise), level=float(level))


def _lo(baud, nyq, eps):         # the tone whose lower band edge is eps * nyq
    return baud + eps * nyq


def _hi(baud, nyq, eps):         # the tone whose upper band edge is (1 - eps) * nyq
    return nyq * (1.0 - eps) - baud


CASES = [
    # ---- lowbaud
    _c("lowbaud", 45.45, 2125, 2295, 96000, 130000, "float32", 101),
    _c("lowbaud", 45.45, 1275, 1445, 48000, 70001, "float64", 102, noise=0.2),
    _c("lowbaud", 50, 1275, 1445, 96000, 122880, "int16", 103),
    _c("lowbaud", 50, 2125, 2295, 48000, 60000, "float32", 104, level=0.01),
    _c("lowbaud", 75, 2125, 2295, 96000, 96000, "float64", 105),
    _c("lowbaud", 75, 1275, 1445, 48000, 40003, "int16", 106, noise=0.2),
    _c("lowbaud", 110, 1275, 1445, 96000, 60000, "float32", 107),
    _c("lowbaud", 110, 2125, 2295, 48000, 30000, "float64", 108, kind="noise"),
    _c("lowbaud", 300, 1200, 2200, 8000, 2000, "int16", 109),
    _c("lowbaud", 300, 1200, 2200, 11025, 3001, "float32", 110),
    _c("lowbaud", 300, 1200, 2200, 22050, 6000, "float64", 111, noise=0.2),
    _c("lowbaud", 1200, 2400, 4800, 192000, 12000, "float32", 112),
    # ---- edge0: the mark band's lower edge a hair above 0, and on it
    _c("edge0", 1200, _lo(1200, 48000.0, 1e-6), 4800, 96000, 8000, "float32", 201),
    _c("edge0", 1200, _lo(1200, 24000.0, 1e-3), 4800, 48000, 4001, "int16", 202),
    _c("edge0", 9600, _lo(9600, 48000.0, 1e-3), 24000, 96000, 3000, "float64", 203, noise=0.2),
    _c("edge0", 2400, _lo(2400, 48000.0, 1e-6), 12000, 96000, 6000, "float64", 204),
    _c("edge0", 300, _lo(300, 24000.0, 1e-6), 1500, 48000, 12000, "float64", 205, kind="noise"),
    _c("edge0", 1200, 1200, 4800, 96000, 4000, "float32", 206),                     # exactly 0: raises
    # ---- edgenyq: the space band's upper edge a hair below Nyquist, and on it
    _c("edgenyq", 1200, 12000, _hi(1200, 48000.0, 1e-6), 96000, 8000, "float32", 301),
    _c("edgenyq", 2400, 6000, _hi(2400, 24000.0, 1e-3), 48000, 4001, "int16", 302),
    _c("edgenyq", 9600, 12000, _hi(9600, 48000.0, 1e-3), 96000, 3000, "float64", 303, noise=0.2),
    _c("edgenyq", 300, 5000, _hi(300, 22050.0, 1e-6), 44100, 12000, "float32", 304, kind="noise"),
    _c("edgenyq", 1200, 12000, 46800, 96000, 4000, "float64", 305),                 # exactly 1: raises
    # ---- same / overlap / swapped
    _c("same", 1200, 6000, 6000, 96000, 8000, "float32", 401),
    _c("same", 9600, 20000, 20000, 96000, 2401, "int16", 402),
    _c("same", 2400, 7000, 7000, 48000, 4000, "float64", 403, kind="noise"),
    _c("overlap", 1200, 6000, 7200, 96000, 8000, "float32", 411),
    _c("overlap", 4800, 12000, 16800, 96000, 3001, "int16", 412, noise=0.2),
    _c("overlap", 300, 2125, 2425, 48000, 12000, "float64", 413, kind="noise"),
    _c("swapped", 1200, 4800, 2400, 96000, 8000, "float32", 421),
    _c("swapped", 9600, 24000, 12000, 96000, 2401, "float64", 422, noise=0.2),
    _c("swapped", 2400, 12000, 5000, 48000, 4000, "int16", 423, kind="noise"),
    # ---- slow: 16 decision bits each (n = 16 samples-per-bit, 5-smooth)
    _c("slow", 1, 96000, 96500, 384000, 16 * 384000, "float32", 501),
    _c("slow", 0.5, 24000, 24100, 96000, 16 * 192000, "int16", 502, noise=0.2),
    _c("slow", 1, 48000, 47000, 192000, 16 * 192000, "float64", 503),
    _c("slow", 0.25, 12000, 12050, 48000, 16 * 192000, "float32", 504, kind="noise"),
    # ---- unstable
    _c("unstable", 10, 30, 50, 96000, 400000, "float32", 601),
    _c("unstable", 10, 40, 70, 96000, 400000, "float64", 602, noise=0.2),
    _c("unstable", 10, 50, 30, 96000, 400000, "int16", 603, kind="noise"),
]
for _i, _case in enumerate(CASES):
    _case["id"] = f"e{_i:02d}_{_case['edge']}"


def make_input(c) -> np.ndarray:
    """The capture of case c (a CASES entry, or its manifest record) from its
    seed: the frame b'FBPC' + random bytes as a CPFSK waveform
    (synth.fsk_waveform: four 0xAA bytes first) after a lead-in of less than a
    bit, cut at n, over a noise floor -- or plain noise (kind 'noise')."""
    import synth
    p = c.get("params", c)
    n, fs, baud = int(c["n"]), p["samp_rate"], p["baud"]
    rng = np.random.default_rng(int(p["seed"]))
    if p["kind"] == "noise":
        x = rng.normal(0.0, 0.3, n)
    else:
        spb = int(round(fs * (1.0 / baud)))
        lead = int(rng.integers(0, spb))
        nbytes = -(-(n - lead) // (8 * spb)) + 1
        data = (b"FBPC" + rng.integers(0, 256, nbytes, dtype=np.uint8).tobytes())[:max(0, nbytes - 4)]
        w = synth.fsk_waveform(data, baud, p["f0"], p["f1"], fs)
        x = np.zeros(n)
        seg = w[:n - lead]
        x[lead:lead + seg.size] = seg * p["level"]
        x += rng.normal(0.0, p["noise"] * p["level"], n)
    if c["dtype"] == "int16":
        return np.round(np.clip(x, -1.0, 1.0) * 32767.0).astype(np.int16)
    return (np.round(x * 32768.0) / 32768.0).astype(c["dtype"])


def sha256(x: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


def stored(x: np.ndarray) -> bool:
    return x.nbytes <= STORE_BYTES


def load():
    """(manifest, stored inputs) of tests/golden/make_fsk_edge_golden.py."""
    import json
    import os
    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    with open(os.path.join(g, "fsk_edge_manifest.json")) as f:
        manifest = json.load(f)
    return manifest, np.load(os.path.join(g, "fsk_edge.npz"))


def case_input(c, npz) -> np.ndarray:
    """Manifest case c's input, regenerated from its seed; the recorded
    SHA-256 (and the stored copy, where there is one) must be this array's, so
    a drift in generation fails here and is not compared against stale bytes."""
    x = make_input(c)
    assert str(x.dtype) == c["dtype"] and x.size == c["n"], c["id"]
    assert sha256(x) == c["sha256"], f"{c['id']}: the regenerated input is not the one the reference saw"
    if c["stored"]:
        assert npz[c["id"]].dtype == x.dtype and np.array_equal(npz[c["id"]], x), c["id"]
    return x


def outcome(fn):
    """("ok", hex) or ("err", exception type, message) -- the manifest's form."""
    try:
        return ("ok", bytes(fn()).hex())
    except Exception as e:      # noqa: BLE001  (the reference's error contract is part of parity)
        return ("err", type(e).__name__, str(e))


def demod(mod, c, x, **kw):
    p = c["params"]
    return mod.fsk_demodulate(x, baud=p["baud"], mark_freq=p["f0"], space_freq=p["f1"], samp_rate=p["samp_rate"], **kw)
