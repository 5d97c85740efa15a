#!/usr/bin/env python3
"""Reference outputs at the edges of the PSK demodulators' parameter space
(needs the reference checkout): the REFERENCE's own modem.qpsk_demodulate /
bpsk_demodulate (modem.py:189-266, 68-135) on the cases of
tests/psk_edge_cases.py -- narrow band-passes at 31.25 .. 110 Bd, designs
whose band-pass output grows (and overflows) by coefficient rounding,
low-passes whose numerator is below 2^-50, band edges clamped at 0.01 / 0.99,
a carrier on fs / 4, 2 and 3 samples per symbol, fractional rates, and the
parameters the reference raises on.  Committed data only:

  tests/golden/psk_edge.npz            the short inputs (their own dtype), key = case id
  tests/golden/psk_edge_manifest.json  per case: parameters (params.edge the
                                       class), dtype, n, the input's SHA-256
                                       and the reference's bytes (hex) or
                                       exception

params.bp_peak / params.bp_nonfinite are the peak over the finite samples and
the count of non-finite samples of scipy's own filtfilt(b, a, x) for the
case's band-pass (modem.py:76-77, 197-198) on the case's input: they DEFINE
the classes grow and overflow (params.lp_b0, the low-pass's b[0], the class
lpsmall), and this script asserts what every class
claims (change a case that misses its class, not the assertion).

Every input is regenerated in the tests from its seed (psk_edge_cases.make_input)
and checked against the recorded SHA-256.  The reference gets each array as
it is -- an int16 capture as raw int16 values, whose odd extension scipy
forms (and wraps) in int16 -- which is what the drop-in's public functions
take.  tests/test_oracle_golden.py pins the oracle to these on the CPU;
tests/test_gpu_psk_edge.py checks the GPU against them.

Run:  python tests/golden/make_psk_edge_golden.py   (the reference at make_golden.REF)
"""
from __future__ import annotations

import io
import json
import os
import sys
import tempfile
import warnings
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (the reference import helpers; its main() is not run)
import psk_edge_cases as ec  # noqa: E402

STABLE = ("lowbaud", "clamp_lo", "clamp_hi", "clamp_both", "quarter", "sps23", "frac")


def bandpass_growth(p, x):
    """(peak over the finite samples, non-finite count) of scipy's filtfilt of
    x through the case's band-pass, designed as modem.py:73-77 / 194-198 do,
    and the low-pass's b[0] (modem.py:86, 203)."""
    from scipy import signal
    nyq = p["samp_rate"] / 2
    half = p["baud"] * (1.5 if p["kind"] == "qpsk" else 1.0)
    b, a = signal.butter(4, [max(0.01, (p["carrier"] - half) / nyq), min(0.99, (p["carrier"] + half) / nyq)],
                         btype="band")
    y = signal.filtfilt(b, a, x)
    fin = np.isfinite(y)
    bl, _ = signal.butter(4, p["baud"] / nyq, btype="low")
    return (float(np.abs(y[fin]).max()) if fin.any() else 0.0), int(y.size - fin.sum()), float(bl[0])


def check_class(c, p, x, res):
    """What the case's class claims (module docstring), or AssertionError."""
    edge, cid = p["edge"], c["id"]
    if edge == "raise":
        assert res["status"] == "err", cid
        return
    assert res["status"] == "ok", (cid, res)
    peak_x = float(np.abs(x.astype(np.float64)).max())
    if edge == "grow":
        assert p["bp_nonfinite"] == 0 and p["bp_peak"] > 1e6 * peak_x, (cid, p["bp_peak"], p["bp_nonfinite"])
    elif edge == "overflow":
        assert p["bp_nonfinite"] > 0, (cid, p["bp_peak"])
    elif edge in STABLE:
        assert len(res["out"]) >= 2 and p["bp_nonfinite"] == 0 and np.isfinite(p["bp_peak"]), (cid, p)
        assert p["bp_peak"] <= 1e3 * peak_x, (cid, p["bp_peak"])      # and not a growing design in disguise
    else:
        assert edge == "lpsmall" and len(res["out"]) >= 2 and 0.0 < p["lp_b0"] < 2.0 ** -50, (cid, p["lp_b0"])


def main():
    scratch = tempfile.mkdtemp(prefix="amr_psk_edge_golden_")
    cwd = os.getcwd()
    try:
        modem, _, _ = mg._import_reference(scratch)
        cases, arrays = [], {}
        for c in ec.CASES:
            x = ec.make_input(c)
            p = {k: c[k] for k in ec.PARAM_KEYS}
            fn = modem.qpsk_demodulate if p["kind"] == "qpsk" else modem.bpsk_demodulate
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                res = mg._run(fn, x, baud=p["baud"], carrier=p["carrier"], samp_rate=p["samp_rate"])
                if res["status"] == "ok":
                    p["bp_peak"], p["bp_nonfinite"], p["lp_b0"] = bandpass_growth(p, x)
            check_class(c, p, x, res)
            if ec.stored(x):
                arrays[c["id"]] = x
            cases.append(dict(id=c["id"], fn=p["kind"], params=p, dtype=str(x.dtype), n=int(x.size),
                              sha256=ec.sha256(x), stored=ec.stored(x), **res))
            print(c["id"], x.dtype, x.size, res["status"], p.get("bp_peak"), p.get("bp_nonfinite"),
                  res.get("out", res.get("emsg", ""))[:48], flush=True)
    finally:
        os.chdir(cwd)
    # a fixed zip timestamp: np.savez stamps the time of writing
    with zipfile.ZipFile(os.path.join(HERE, "psk_edge.npz"), "w", zipfile.ZIP_DEFLATED) as z:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, arrays[k], allow_pickle=False)
            z.writestr(zipfile.ZipInfo(k + ".npy", (1980, 1, 1, 0, 0, 0)), buf.getvalue(), zipfile.ZIP_DEFLATED)
    head = json.dumps({"generator": "tests/golden/make_psk_edge_golden.py", "numpy": np.__version__,
                       "numpy_cpu_features": mg.numpy_cpu_features()})
    with open(os.path.join(HERE, "psk_edge_manifest.json"), "w") as f:      # one case per line
        f.write(head[:-1] + ', "cases": [\n' + ",\n".join(json.dumps(c) for c in cases) + "\n]}\n")
    ok = sum(c["status"] == "ok" for c in cases)
    print(f"{len(cases)} cases ({ok} ok, {len(cases) - ok} raise), {len(arrays)} inputs stored")


if __name__ == "__main__":
    main()
