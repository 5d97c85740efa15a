"""PSK captures at the edges of qpsk_demodulate's / bpsk_demodulate's
parameter space (the reference's modem.py:68-135, 189-266 accept all of them):
the case list of tests/golden/make_psk_edge_golden.py and the seeded generator
of its inputs.

Classes (params.edge in tests/golden/psk_edge_manifest.json):
  lowbaud     narrow, stable band-passes: 31.25 (PSK31), 45.45, 50, 75, 110 Bd
              at 8 / 11.025 / 48 / 96 kHz
  grow        butter(4, band)'s transfer-function form is unstable by
              coefficient rounding: scipy's own filtfilt output grows past
              1e6 max|x| but stays finite at this length (params.bp_peak,
              params.bp_nonfinite -- measured, not predicted from the poles)
  overflow    the same designs at a length where that output holds inf / NaN;
              the reference decides its bytes from them
  lpsmall     butter(4, baud / nyq)'s b[0] < 2^-50 (params.lp_b0; 5 and 1 Bd at
              96 kHz, 2 Bd at 48 kHz): the plan's low-pass is exact-only by
              design.  One of them on a band-pass that overflows, three on
              carriers high enough for a stable one
  clamp_lo / clamp_hi / clamp_both
              a band edge clamped at 0.01, at 0.99, or both (modem.py:76, 197)
  quarter     carrier = samp_rate / 4: the band-pass's odd denominator taps
              are rounding residue (1e-16), not zeros
  sps23       2 and 3 samples per symbol, and the two sides of int(fs / baud)
  frac        fractional baud, fractional sample rate, 1200 Bd at 44.1 kHz
  raise       scipy's ValueError texts and baud 0's ZeroDivisionError

Most inputs are too long to commit, so every input is regenerated from its
seed (make_input) and checked against the SHA-256 the manifest recorded when
the reference ran; the short ones are also stored (psk_edge.npz).  Samples sit
on the 2^-15 grid (floats) or are int16, so a last-ulp difference in a host's
sin / normal does not move them.  Lengths are the shortest that give a byte
or a few, except that a third of the stable cases are long enough (four
warm-ups, csrc/api.cpp split_design_core) to have a time-split design.  baud, carrier and samp_rate keep the Python
type written here (int / int is the reference's 'division by zero')."""
from __future__ import annotations

import hashlib

import numpy as np

STORE_BYTES = 48 * 1024          # inputs up to this size are also stored in psk_edge.npz


def _c(edge, kind, baud, carrier, fs, n, dtype, seed, sig="frame", noise=0.05, level=1.0):
    return dict(edge=edge, kind=kind, baud=baud, carrier=carrier, samp_rate=fs, n=int(n), dtype=dtype,
                seed=int(seed), kind_of_signal=sig, noise=float(noise), level=float(level))


CASES = [
    # ---- lowbaud: stable narrow designs
    _c("lowbaud", "bpsk", 31.25, 1000.0, 8000, 6000, "float32", 101),
    _c("lowbaud", "qpsk", 31.25, 1500.0, 48000, 40001, "float64", 102, noise=0.2),
    _c("lowbaud", "qpsk", 31.25, 2000.0, 96000, 61440, "int16", 103),
    _c("lowbaud", "bpsk", 45.45, 1200.0, 11025, 20001, "int16", 104, noise=0.2),
    _c("lowbaud", "qpsk", 45.45, 1500.0, 96000, 50000, "float64", 105),
    _c("lowbaud", "bpsk", 50, 1500.0, 48000, 30000, "float32", 106, level=0.01),
    _c("lowbaud", "qpsk", 75, 1000.0, 8000, 8003, "int16", 107),
    _c("lowbaud", "bpsk", 75, 3000.0, 96000, 40000, "float64", 108, sig="noise"),
    _c("lowbaud", "qpsk", 110, 1275.0, 11025, 8000, "float32", 109, noise=0.2),
    _c("lowbaud", "bpsk", 110, 2125.0, 96000, 64000, "int16", 110),
    # ---- grow: scipy's band-pass output grows and stays finite
    _c("grow", "bpsk", 31.25, 1000.0, 96000, 130000, "float32", 201),
    _c("grow", "bpsk", 31.25, 1000.0, 96000, 1500000, "float64", 202, noise=0.2),
    _c("grow", "bpsk", 50, 500.0, 96000, 60000, "int16", 203),
    _c("grow", "qpsk", 300, 100.0, 96000, 8000, "float32", 204),
    _c("grow", "qpsk", 300, 100.0, 96000, 30000, "float64", 205, sig="noise"),
    _c("grow", "qpsk", 6, 1000.0, 96000, 400000, "float32", 206),
    # ---- overflow: the same designs where it reaches inf / NaN
    _c("overflow", "bpsk", 50, 500.0, 96000, 300000, "float64", 301),
    _c("overflow", "qpsk", 300, 100.0, 96000, 200000, "float32", 302, noise=0.2),
    _c("overflow", "qpsk", 10, 1000.0, 96000, 400000, "int16", 303),
    # ---- lpsmall: the low-pass numerator below 2^-50
    _c("lpsmall", "qpsk", 5, 1000.0, 96000, 400000, "float32", 401),
    _c("lpsmall", "bpsk", 2, 21000.0, 48000, 220000, "float64", 402),
    _c("lpsmall", "qpsk", 1, 30000.0, 96000, 500000, "int16", 403),
    _c("lpsmall", "bpsk", 5, 36000.0, 96000, 200000, "float32", 404, sig="noise"),
    # ---- clamp_lo / clamp_hi / clamp_both
    _c("clamp_lo", "qpsk", 300, 500.0, 96000, 8000, "float32", 501),
    _c("clamp_lo", "qpsk", 9600, 1800.0, 96000, 1201, "int16", 502, noise=0.2),
    _c("clamp_lo", "bpsk", 1200, 1000.0, 96000, 24000, "float64", 503),
    _c("clamp_hi", "bpsk", 1200, 47000.0, 96000, 24001, "float64", 511),
    _c("clamp_hi", "qpsk", 1200, 47500.0, 96000, 4000, "float32", 512, noise=0.2),
    _c("clamp_hi", "qpsk", 2400, 48000.0, 96000, 3000, "int16", 513),
    _c("clamp_both", "qpsk", 19200, 12000.0, 44100, 16000, "float32", 521),
    _c("clamp_both", "bpsk", 30000, 24000.0, 96000, 1501, "float64", 522),
    _c("clamp_both", "qpsk", 24000, 20000.0, 96000, 1200, "int16", 523),
    # ---- quarter: carrier = fs / 4
    _c("quarter", "qpsk", 9600, 24000.0, 96000, 2000, "float32", 601),
    _c("quarter", "bpsk", 1200, 12000.0, 48000, 3001, "int16", 602, noise=0.2),
    _c("quarter", "qpsk", 1200, 11025.0, 44100, 4000, "float64", 603),
    # ---- sps23
    _c("sps23", "qpsk", 47999, 12000.0, 96000, 400, "float32", 701),
    _c("sps23", "qpsk", 22000, 6000.0, 44100, 601, "float64", 702),
    _c("sps23", "bpsk", 19200, 3000.0, 44100, 14001, "int16", 703),
    _c("sps23", "qpsk", 31999.9, 12000.0, 96000, 14000, "float64", 704),
    _c("sps23", "qpsk", 32000.1, 12000.0, 96000, 701, "float32", 705),
    _c("sps23", "bpsk", 47999, 20000.0, 96000, 300, "float32", 706),
    # ---- frac
    _c("frac", "qpsk", 1200.5, 3000.0, 96000, 12000, "float32", 801),
    _c("frac", "bpsk", 1200, 3000.0, 96000.5, 8001, "float64", 802, noise=0.2),
    _c("frac", "qpsk", 1200, 3000.0, 44100, 6000, "int16", 803),
    # ---- raise: the reference's error contract
    _c("raise", "bpsk", 100, 200.0, 96000, 4000, "float32", 901),          # Wn[0] must be less than Wn[1]
    _c("raise", "qpsk", 2400, 60000.0, 96000, 4000, "float64", 902),       # both edges 0.99
    _c("raise", "qpsk", 300, 0, 96000, 4000, "float32", 903),              # carrier 0: the upper edge below 0.01
    _c("raise", "bpsk", -1200, 3000.0, 96000, 4000, "int16", 904),         # negative baud: the edges swap
    _c("raise", "qpsk", 300, -500.0, 96000, 4000, "float32", 905),         # upper edge below 0
    _c("raise", "qpsk", 48000, 3000.0, 96000, 4000, "float64", 906),       # baud on Nyquist: the low-pass design
    _c("raise", "bpsk", 100000, 3000.0, 96000, 4000, "float32", 907),      # baud > fs: sps 0
    _c("raise", "qpsk", 0, 3000.0, 96000, 4000, "float32", 908),           # int / 0
]
for _i, _case in enumerate(CASES):
    _case["id"] = f"p{_i:02d}_{_case['edge']}_{_case['kind']}"

PARAM_KEYS = ("edge", "kind", "baud", "carrier", "samp_rate", "seed", "kind_of_signal", "noise", "level")


def _sps(fs, baud) -> int:
    try:
        return int(fs / baud)
    except ZeroDivisionError:
        return 0


def make_input(c) -> np.ndarray:
    """The capture of case c (a CASES entry, or its manifest record) from its
    seed: the frame b'FBPC' + random bytes as synth.qpsk_waveform /
    bpsk_waveform (their preambles first) after a lead-in of less than a
    symbol, cut at n, over a noise floor -- or plain noise (kind_of_signal
    'noise', and below 10 samples per symbol, where the reference's modulator
    raises)."""
    import synth
    p = c.get("params", c)
    n, fs, baud = int(c["n"]), p["samp_rate"], p["baud"]
    rng = np.random.default_rng(int(p["seed"]))
    sps = _sps(fs, baud)
    if p["kind_of_signal"] == "noise" or sps < 10:
        x = rng.normal(0.0, 0.3, n)
    else:
        lead = int(rng.integers(0, sps))
        per_byte, pre = (4, 40) if p["kind"] == "qpsk" else (8, 80)
        nsym = -(-(n - lead) // sps)
        nbytes = max(0, -(-(nsym - pre) // per_byte)) + 1
        data = (b"FBPC" + rng.integers(0, 256, nbytes, dtype=np.uint8).tobytes())[:nbytes]
        wave = synth.qpsk_waveform if p["kind"] == "qpsk" else synth.bpsk_waveform
        w = wave(data, baud, p["carrier"], fs)
        x = np.zeros(n)
        seg = w[:n - lead]
        x[lead:lead + seg.size] = seg.astype(np.float64) * p["level"]
        x += rng.normal(0.0, p["noise"] * p["level"], n)
    if c["dtype"] == "int16":
        return np.round(np.clip(x, -1.0, 1.0) * 32767.0).astype(np.int16)
    return (np.round(x * 32768.0) / 32768.0).astype(c["dtype"])


def sha256(x: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()


def stored(x: np.ndarray) -> bool:
    return x.nbytes <= STORE_BYTES


_LOADED = None


def load():
    """(manifest, stored inputs) of tests/golden/make_psk_edge_golden.py."""
    global _LOADED
    if _LOADED is None:
        import json
        import os
        g = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
        with open(os.path.join(g, "psk_edge_manifest.json")) as f:
            manifest = json.load(f)
        _LOADED = manifest, np.load(os.path.join(g, "psk_edge.npz"))
    return _LOADED


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


def expected(c):
    return ("ok", c["out"]) if c["status"] == "ok" else ("err", c["etype"], c["emsg"])


def _normal(v) -> bool:
    return bool(np.isfinite(v) and abs(v) >= np.finfo(np.float64).tiny)


def bp_zero_odd(bp) -> bool:
    """amr_psk_plan_create's predicate (csrc/api.cpp) on design_psk's band-pass
    (b, a, zi): the odd b taps are +0, every odd a tap finite and >= 2^-40."""
    b, a, _ = bp
    return (all(v == 0.0 and not np.signbit(v) for v in b[1::2])
            and all(np.isfinite(v) and abs(v) >= 2.0 ** -40 for v in a[1::2]))


def lp_exact_only(lp) -> bool:
    """amr_psk_plan_create's predicate on design_psk's low-pass (b, a, zi): a b
    that is not positive, normal and >= 2^-50, or an a / zi that is not normal."""
    b, a, zi = lp
    return not (all(v > 0.0 and _normal(v) and v >= 2.0 ** -50 for v in b)
                and all(_normal(v) for v in a[1:]) and all(_normal(v) for v in zi))


def lp_palindromic(lp) -> bool:
    """pick_layout's condition for the lane kernels: butter's b[4] == b[0], b[3] == b[1], bit for bit."""
    b = lp[0]
    return len(b) == 5 and b[4].tobytes() == b[0].tobytes() and b[3].tobytes() == b[1].tobytes()


def demod(mod, c, x, **kw):
    p = c["params"]
    f = mod.qpsk_demodulate if p["kind"] == "qpsk" else mod.bpsk_demodulate
    return f(x, baud=p["baud"], carrier=p["carrier"], samp_rate=p["samp_rate"], **kw)
