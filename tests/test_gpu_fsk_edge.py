"""The FSK drop-in at the edges of fsk_demodulate's parameter space, against
the REFERENCE's own bytes (tests/golden/make_fsk_edge_golden.py, cases and
inputs: tests/fsk_edge_cases.py): narrow band-passes at low and non-integer
baud, a band edge 1e-6 / 1e-3 from 0 or Nyquist (and on it: the reference's
ValueError), mark == space, half-overlapping and swapped tone bands,
band-passes whose responses outlast the walk behind F2's FFT rounding bound
(csrc/fsk_api.cpp fsk_fft_bound: such a plan sends every stream through the
exact path) and designs whose transfer-function form is
unstable (the reference decides from inf / NaN envelopes).

Every case one capture per call (the reference's call pattern), and every
decodable case again as the middle row of a batch of 3 between two unrelated
captures of the same length, whose bytes are the oracle's
(tests/test_oracle_golden.py pins the oracle to this fixture on the CPU)."""
import warnings

import numpy as np
import pytest

import fsk_edge_cases as ec

pytestmark = pytest.mark.gpu

MANIFEST, STORED = ec.load()
CASES = MANIFEST["cases"]
# no FFT rounding bound for these filters (tests/test_fsk_fft_bound.py): every stream goes exact
NO_BOUND = {c["id"] for c in CASES if c["params"]["edge"] in ("slow", "unstable")} | {
    "e12_edge0", "e15_edge0", "e16_edge0", "e18_edgenyq", "e21_edgenyq"}


@pytest.fixture(scope="module", autouse=True)
def gpu(built_lib):
    import _amr
    if _amr.device_count() < 1:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X")


def _expected(c):
    return ("ok", c["out"]) if c["status"] == "ok" else ("err", c["etype"], c["emsg"])


def _plan(c, B):
    import _fsk
    p = c["params"]
    return _fsk.get_fsk_plan(c["n"], p["baud"], p["f0"], p["f1"], p["samp_rate"], B)


def test_manifest_covers_every_class():
    edges = [c["params"]["edge"] for c in CASES]
    assert set(edges) == {"lowbaud", "edge0", "edgenyq", "same", "overlap", "swapped", "slow", "unstable"}
    ok = sum(c["status"] == "ok" for c in CASES)
    assert len(CASES) >= 39 and ok > len(CASES) - ok
    assert [c["emsg"] for c in CASES if c["status"] != "ok" and c["params"]["edge"] in ("edge0", "edgenyq")]
    for c in CASES:
        if c["params"]["edge"] == "unstable":
            assert c["params"]["max_pole"] > 1.0, c["id"]
        if c["params"]["edge"] == "slow":
            assert c["params"]["max_pole"] < 1.0 and c["n"] >= 16 * int(c["params"]["samp_rate"] / c["params"]["baud"])


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_drop_in_gives_the_references_bytes(case):
    import modem
    x = ec.case_input(case, STORED)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                   # scipy's BadCoefficients on the near-singular designs
        got = ec.outcome(lambda: ec.demod(modem, case, x))
    assert got == _expected(case), (case["id"], case["params"])
    if case["status"] != "ok":
        return
    pl = _plan(case, 1)
    if case["params"]["edge"] == "same":
        # both envelopes equal: every compare is a tie inside F2's margin
        assert pl.exact_streams() >= 1
    if case["id"] in NO_BOUND:
        assert pl.exact_streams() == 1 and not np.isfinite(pl.margin()["tau"])


@pytest.mark.parametrize("case", [c for c in CASES if c["status"] == "ok"], ids=lambda c: c["id"])
def test_batch_rows_do_not_leak(case):
    """The case between two unrelated rows (another frame at another seed and
    level, and plain noise) in one call: the middle row's bytes are still the
    reference's and the neighbours' the oracle's -- the exact path's
    per-stream flags and bits belong to their own row."""
    import modem
    from oracle import oracle
    p = case["params"]
    x = ec.case_input(case, STORED)
    a = ec.make_input(dict(case, params=dict(p, seed=p["seed"] + 5000, kind="frame", level=0.5, noise=0.3)))
    b = ec.make_input(dict(case, params=dict(p, seed=p["seed"] + 6000, kind="noise")))
    batch = np.stack([a, x, b])
    assert batch.dtype == x.dtype
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        want = [ec.demod(oracle, case, a, raw_int16=True).hex(), case["out"],
                ec.demod(oracle, case, b, raw_int16=True).hex()]
        got = modem.fsk_demodulate_batch(batch, baud=p["baud"], mark_freq=p["f0"], space_freq=p["f1"],
                                         samp_rate=p["samp_rate"])
    assert [g.hex() for g in got] == want, (case["id"], p)
    pl = _plan(case, 3)
    if p["edge"] == "same":
        assert pl.exact_streams() >= 1
    if case["id"] in NO_BOUND:
        assert pl.exact_streams() == 3
