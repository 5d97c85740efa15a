#!/usr/bin/env python3
"""Reference outputs at the edges of fsk_demodulate's parameter space (needs
the reference checkout): the REFERENCE's own modem.fsk_demodulate (modem.py:298-341)
on the cases of tests/fsk_edge_cases.py -- narrow band-passes at low baud, a
band edge a hair from 0 or Nyquist (and on it, where scipy raises), equal,
overlapping and swapped tone bands, band-passes too slow for the library's
FFT rounding bound, and designs whose transfer-function form is unstable.
Committed data only:

  tests/golden/fsk_edge.npz            the short inputs (their own dtype), key = case id
  tests/golden/fsk_edge_manifest.json  per case: parameters (params.edge the
                                       class), dtype, n, the input's SHA-256
                                       and the reference's bytes (hex) or
                                       exception

Every input is regenerated in the tests from its seed (fsk_edge_cases.make_input)
and checked against the recorded SHA-256.  The reference gets each array as
it is -- an int16 capture as raw int16 values, whose odd extension scipy
forms (and wraps) in int16 -- which is what the drop-in's public functions
take.  tests/test_oracle_golden.py pins the oracle to these on the CPU;
tests/test_gpu_fsk_edge.py checks the GPU against them.

Run:  python tests/golden/make_fsk_edge_golden.py   (the reference at make_golden.REF)
"""
from __future__ import annotations

import json
import os
import sys
import tempfile
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (the reference import helpers; its main() is not run)
import fsk_edge_cases as ec  # noqa: E402


def max_pole(baud, f, fs) -> float:
    """max |pole| of butter(3, band)'s denominator as scipy returns it."""
    from scipy import signal
    nyq = fs / 2
    _, a = signal.butter(3, [(f - baud) / nyq, (f + baud) / nyq], btype="band")
    return float(np.abs(np.roots(a)).max())


def main():
    scratch = tempfile.mkdtemp(prefix="amr_fsk_edge_golden_")
    cwd = os.getcwd()
    try:
        modem, _, _ = mg._import_reference(scratch)
        cases, arrays = [], {}
        for c in ec.CASES:
            x = ec.make_input(c)
            p = {k: c[k] for k in ("edge", "baud", "f0", "f1", "samp_rate", "seed", "kind", "noise", "level")}
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                res = mg._run(modem.fsk_demodulate, x, baud=p["baud"], mark_freq=p["f0"], space_freq=p["f1"],
                              samp_rate=p["samp_rate"])
            if res["status"] == "ok":
                p["max_pole"] = max(max_pole(p["baud"], f, p["samp_rate"]) for f in (p["f0"], p["f1"]))
            if ec.stored(x):
                arrays[c["id"]] = x
            cases.append(dict(id=c["id"], fn="fsk", params=p, dtype=str(x.dtype), n=int(x.size),
                              sha256=ec.sha256(x), stored=ec.stored(x), **res))
            print(c["id"], x.dtype, x.size, res["status"], res.get("out", res.get("emsg", ""))[:48], flush=True)
    finally:
        os.chdir(cwd)
    np.savez_compressed(os.path.join(HERE, "fsk_edge.npz"), **arrays)
    head = json.dumps({"generator": "tests/golden/make_fsk_edge_golden.py", "numpy": np.__version__,
                       "numpy_cpu_features": mg.numpy_cpu_features()})
    with open(os.path.join(HERE, "fsk_edge_manifest.json"), "w") as f:      # one case per line
        f.write(head[:-1] + ', "cases": [\n' + ",\n".join(json.dumps(c) for c in cases) + "\n]}\n")
    ok = sum(c["status"] == "ok" for c in cases)
    print(f"{len(cases)} cases ({ok} ok, {len(cases) - ok} raise), {len(arrays)} inputs stored")


if __name__ == "__main__":
    main()
