"""The PSK plan's design branches at the edges of the parameter space
(tests/psk_edge_cases.py, fixtures of tests/golden/make_psk_edge_golden.py):
pure host arithmetic in libamr.so -- _amr.design_psk, split_design,
split_strict_design, f32_margin -- no device.

amr_psk_plan_create (csrc/api.cpp) picks three branches from the coefficients
alone; its predicates are restated in psk_edge_cases.py so that the fixture is known to hold
each outcome, by design and not through an environment hook:
  bp_zero_odd   the band-pass's odd b taps are +0 and every odd a tap is
                finite and at least 2^-40 (off: carrier on fs / 4, or both
                band edges clamped)
  lp_exact_only a low-pass b below 2^-50 or not normal, or an a / zi that is
                not normal (on: 5, 2 and 1 Bd)
  split design  split_design_core: both filters' responses decay, and the
                warm-ups fit in n / 4 (refused: every growing or overflowing
                band-pass, every exact-only low-pass, every short capture)"""
import math
import time
import warnings

import numpy as np
import pytest

import psk_edge_cases as ec

MANIFEST, STORED = ec.load()
CASES = MANIFEST["cases"]
OK = [c for c in CASES if c["status"] == "ok"]
CLASSES = {"lowbaud", "grow", "overflow", "lpsmall", "clamp_lo", "clamp_hi", "clamp_both", "quarter", "sps23",
           "frac", "raise"}


def _args(c):
    p = c["params"]
    return p["kind"], c["n"], p["baud"], p["carrier"], p["samp_rate"]


@pytest.fixture(scope="module")
def designs(built_lib):
    """Per decodable case: (design_psk's result, split_design, split_strict_design, f32_margin, seconds)."""
    import _amr
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                   # scipy's BadCoefficients on the near-singular designs
        for c in OK:
            t0 = time.perf_counter()
            d = _amr.design_psk(*_args(c))
            sd, ss, m = _amr.split_design(*_args(c)), _amr.split_strict_design(*_args(c)), _amr.f32_margin(*_args(c))
            out[c["id"]] = (d, sd, ss, m, time.perf_counter() - t0)
    return out


def test_manifest_is_complete():
    assert {c["params"]["edge"] for c in CASES} == CLASSES
    assert len(CASES) >= 40 and len(OK) > len(CASES) - len(OK)
    assert [c["id"] for c in CASES] == [c["id"] for c in ec.CASES]
    for a, b in zip(CASES, ec.CASES):
        assert a["n"] == b["n"] and a["dtype"] == b["dtype"] and all(a["params"][k] == b[k] for k in ec.PARAM_KEYS)
        assert type(a["params"]["baud"]) is type(b["baud"]) and type(a["params"]["samp_rate"]) is type(b["samp_rate"])
    errs = {(c["etype"], c["emsg"]) for c in CASES if c["status"] != "ok"}
    assert {t for t, _ in errs} == {"ValueError", "ZeroDivisionError"}
    for text in ("Wn[0] must be less than Wn[1]", "filter critical frequencies must be greater than 0",
                 "Digital filter critical frequencies must be 0 < Wn < 1", "division by zero"):
        assert any(m == text for _, m in errs), text
    for edge in CLASSES:
        cs = [c for c in CASES if c["params"]["edge"] == edge]
        assert {c["params"]["kind"] for c in cs} == {"qpsk", "bpsk"}, edge
    assert {c["dtype"] for c in OK} == {"float32", "float64", "int16"}


def test_manifest_classes_hold():
    """What the generator asserted when the reference ran, from the recorded figures."""
    for c in CASES:
        p = c["params"]
        if p["edge"] == "raise":
            assert c["status"] == "err", c["id"]
            continue
        assert c["status"] == "ok" and len(c["out"]) >= 2, c["id"]
        if p["edge"] == "grow":
            assert p["bp_nonfinite"] == 0 and p["bp_peak"] > 1e6 * (32767 if c["dtype"] == "int16" else 4.0), c["id"]
        elif p["edge"] == "overflow":
            assert p["bp_nonfinite"] > 0, c["id"]
        elif p["edge"] == "lpsmall":
            assert 0.0 < p["lp_b0"] < 2.0 ** -50, c["id"]
        else:
            assert p["bp_nonfinite"] == 0 and p["bp_peak"] < 1e3 * (32767 if c["dtype"] == "int16" else 4.0), c["id"]


def test_every_design_is_finite_or_refused(designs):
    for c in OK:
        (sps, first, bp, lp, _), sd, ss, m, secs = designs[c["id"]]
        assert secs < 5.0, (c["id"], secs)
        assert sps == int(c["params"]["samp_rate"] / c["params"]["baud"]) and sps >= 1
        assert all(np.isfinite(v).all() for v in bp[:2] + lp[:2]), c["id"]
        assert math.isfinite(m) and m >= 0.0, (c["id"], m)
        if sd is not None:
            assert math.isfinite(sd["kappa"]) and sd["kappa"] > 0.0, (c["id"], sd)
            assert 0 < sd["warmup_bp"] <= c["n"] // 4 and 0 < sd["warmup_lp"] <= c["n"] // 4, (c["id"], sd)
        else:
            assert ss is None, c["id"]                   # no strict bound without a split design
        if ss is not None:
            assert math.isfinite(ss["kappa"]) and ss["kappa"] > 0.0, c["id"]
            assert all(np.isfinite(ss[k]).all() for k in ("kabs", "z0abs", "lpc", "W", "K12", "HS", "GS", "TZ")), c["id"]


def test_no_time_split_design_where_the_response_does_not_decay(designs):
    for c in OK:
        if c["params"]["edge"] in ("grow", "overflow", "lpsmall"):
            assert designs[c["id"]][1] is None and designs[c["id"]][2] is None, c["id"]


def test_every_branch_is_held_by_design(designs):
    zodd_off = [c["id"] for c in OK if not ec.bp_zero_odd(designs[c["id"]][0][2])]
    lpx = [c["id"] for c in OK if ec.lp_exact_only(designs[c["id"]][0][3])]
    split = [c["id"] for c in OK if designs[c["id"]][1] is not None]
    refused = [c["id"] for c in OK if designs[c["id"]][1] is None]
    strict = [c["id"] for c in OK if designs[c["id"]][2] is not None]
    edge = {c["id"]: c["params"]["edge"] for c in OK}
    assert sum(edge[i] == "quarter" for i in zodd_off) >= 2 and sum(edge[i] == "clamp_both" for i in zodd_off) >= 2
    assert sorted(lpx) == sorted(i for i in edge if edge[i] == "lpsmall") and len(lpx) >= 2
    assert len(split) >= 5 and len(refused) >= 5 and len(strict) >= 2
    # refused for each of the three reasons: a short capture of a decaying design too
    assert sum(edge[i] not in ("grow", "overflow", "lpsmall") for i in refused) >= 5
    # the ordinary branches are held too: zero odd taps kept, the separable low-pass allowed
    assert len(OK) - len(zodd_off) >= 5 and len(OK) - len(lpx) >= 5
    # bp_zero_odd is off through the a taps alone (1e-16 residue): the b taps are exact zeros everywhere
    for c in OK:
        assert all(v == 0.0 and not np.signbit(v) for v in designs[c["id"]][0][2][0][1::2]), c["id"]


def test_raising_cases_raise_in_the_design():
    """The host design alone (no device) gives the reference's exception."""
    import _amr
    for c in CASES:
        if c["status"] == "ok":
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = ec.outcome(lambda: _amr.design_psk(*_args(c)) and b"")
        assert got == ec.expected(c), c["id"]
