"""The PSK demodulators at the edges of their parameter space, in every device
layout, against the REFERENCE's own bytes (tests/golden/make_psk_edge_golden.py,
cases and inputs: tests/psk_edge_cases.py): 31.25 .. 110 Bd band-passes,
band-passes whose output grows to 1e248 or overflows to inf / NaN by
coefficient rounding (the reference decides its bytes from those values, so
parity means the same bytes), low-passes with b[0] < 2^-50, band edges clamped
at 0.01 / 0.99, a carrier on fs / 4, 2 and 3 samples per symbol, fractional
rates, and the parameters the reference raises on.

Every case one capture through the drop-in (the reference's call pattern);
every decodable case again as the middle row of a batch of 3 between two
unrelated captures, through a plan forced to each layout -- the neighbours'
bytes and all sync indices are the oracle's (tests/test_oracle_golden.py pins
the oracle to this fixture on the CPU); and a growing design's capture at both
ends of a batch of 65 quiet rows.  Every comparison is of bytes: no tolerances.

The path each layout must take, read from csrc/api.cpp:
  pick_layout      a forced 'split' runs the time-split kernels only with a
                   split design (split_design_core) and falls back to 'row';
                   a forced 'lane' needs butter's palindromic low-pass numerator
  split_params     the strict bound runs only with a strict design
  run_psk_row / run_psk_lane
                   an exact-only low-pass (amr_psk_plan_create: b < 2^-50) flags
                   every stream for K3x and launches no separable low-pass, so
                   exact_streams() is the batch and last_lowpass() 'none'
  psk_kernels.hip (K2q / K3q final-state test), psk_lane_kernels.hip
                   a non-finite band-pass output is sticky in the separable
                   low-pass's state and flags its stream: the overflow cases
                   have at least one exact stream.  The grow cases' values are
                   finite, so nothing is implied for them but the layout."""
import functools
import warnings

import numpy as np
import pytest

import psk_edge_cases as ec

pytestmark = pytest.mark.gpu

MANIFEST, STORED = ec.load()
CASES = MANIFEST["cases"]
OK = [c for c in CASES if c["status"] == "ok"]
LAYOUTS = ("row", "lane", "split", "split_strict")
LEAK_IDS = ("p12_grow_bpsk", "p13_grow_qpsk", "p14_grow_qpsk")      # band-pass peaks 7e198 (int16), 9e20, 1e94


@pytest.fixture(scope="module", autouse=True)
def gpu(built_lib):
    import _amr
    if _amr.device_count() < 1:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X")


def _args(c):
    p = c["params"]
    return p["kind"], c["n"], p["baud"], p["carrier"], p["samp_rate"]


def _oracle_batch(c, batch):
    from oracle import oracle
    p = c["params"]
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        outs, sync = oracle.psk_demod_batch(p["kind"], batch, p["baud"], p["carrier"], p["samp_rate"], n_threads=16,
                                            raw_int16=True)
    return [o.hex() for o in outs], [int(s) for s in sync]


@functools.lru_cache(maxsize=2)           # (the layouts of a case run back to back)
def _batch3(cid):
    """(batch [3][n], the oracle's bytes, its sync indices, the host designs) of a case, made once for
    the four layouts: the case between another frame (another seed and level) and plain noise."""
    import _amr
    c = next(k for k in OK if k["id"] == cid)
    p = c["params"]
    x = ec.case_input(c, STORED)
    a = ec.make_input(dict(c, params=dict(p, seed=p["seed"] + 5000, kind_of_signal="frame", level=0.5, noise=0.3)))
    b = ec.make_input(dict(c, params=dict(p, seed=p["seed"] + 6000, kind_of_signal="noise")))
    batch = np.stack([a, x, b])
    assert batch.dtype == x.dtype
    batch.setflags(write=False)
    outs, sync = _oracle_batch(c, batch)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        lp = _amr.design_psk(*_args(c))[3]
        des = dict(split=_amr.split_design(*_args(c)) is not None,
                   strict=_amr.split_strict_design(*_args(c)) is not None,
                   lp_sym=ec.lp_palindromic(lp), lp_exact=ec.lp_exact_only(lp))
    return batch, outs, sync, des


def _run(c, batch, layout):
    import _amr
    B = batch.shape[0]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                   # scipy's BadCoefficients on the near-singular designs
        pl = _amr.PskPlan(*_args(c), max_streams=B)
    pl.set_layout("split" if layout == "split_strict" else layout)
    if layout == "lane":
        pl.set_inflight(max(1, 16384 // B + 1))
    if layout == "split_strict":
        pl.set_split_strict(True)
    outs, sync = pl.demod_host_raw(batch) if batch.dtype == np.int16 else pl.demod_host(batch)
    return pl, [o.hex() for o in outs], [int(s) for s in sync]


def test_manifest_covers_every_class():
    assert {c["params"]["edge"] for c in CASES} == {"lowbaud", "grow", "overflow", "lpsmall", "clamp_lo", "clamp_hi",
                                                   "clamp_both", "quarter", "sps23", "frac", "raise"}
    assert len(CASES) >= 40 and len(OK) > len(CASES) - len(OK)
    assert all(any(c["id"] == i and c["params"]["edge"] == "grow" for c in OK) for i in LEAK_IDS)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c["id"])
def test_drop_in_gives_the_references_bytes(case):
    import modem
    x = ec.case_input(case, STORED)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        got = ec.outcome(lambda: ec.demod(modem, case, x))
    assert got == ec.expected(case), (case["id"], case["params"])


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", OK, ids=lambda c: c["id"])
def test_every_layout(case, layout):
    """The case between two unrelated rows in one call through a plan forced
    to `layout`: the middle row's bytes are the reference's, the neighbours'
    bytes and the three sync indices the oracle's, and the call took the path
    the design implies (module docstring; csrc/api.cpp pick_layout,
    split_params, run_psk_row, run_psk_lane)."""
    batch, want, want_sync, des = _batch3(case["id"])
    assert want[1] == case["out"], case["id"]             # (the oracle pin, on this very batch)
    pl, got, sync = _run(case, batch, layout)
    edge = case["params"]["edge"]
    print(case["id"], layout, "->", pl.last_layout(), "strict", pl.last_strict(), "lowpass", pl.last_lowpass(),
          "exact", pl.exact_streams(), "flagged", pl.split_info()["flagged"])
    assert got == want and sync == want_sync, (case["id"], layout, pl.last_layout(), case["params"])
    if layout == "row":
        took = "row"
    elif layout == "lane":
        took = "lane" if des["lp_sym"] else "row"
    else:
        took = "split" if des["split"] else "row"
    assert pl.last_layout() == took, (case["id"], layout, pl.last_layout())
    assert pl.last_strict() == (layout == "split_strict" and took == "split" and des["strict"]), (case["id"], layout)
    info = pl.split_info()
    if took == "split":
        assert 0 <= info["flagged"] <= 3 and info["warmup_bp"] > 0 and info["kappa"] > 0.0
    else:
        assert info["flagged"] == -1
    if edge in ("grow", "overflow", "lpsmall"):
        assert took != "split" and not des["split"], case["id"]
    if des["lp_exact"]:
        assert edge == "lpsmall" and pl.exact_streams() == 3 and pl.last_lowpass() == "none", case["id"]
    else:
        assert edge != "lpsmall"
        assert (pl.last_lowpass() != "none") == (took == "lane"), (case["id"], layout, pl.last_lowpass())
    if edge == "overflow":
        assert pl.exact_streams() >= 1, case["id"]


@pytest.mark.parametrize("layout", ("lane", "row"))
@pytest.mark.parametrize("cid", LEAK_IDS)
def test_grown_values_do_not_leak(cid, layout):
    """65 rows on a growing design: rows 0 and 64 the case, the 63 between
    them quiet noise at 1e-3 of full scale.  A wave whose neighbour lanes hold
    1e94 .. 1e198 must leave the quiet rows' bytes and sync as the oracle has
    them, and the per-stream flags must belong to their own row."""
    c = next(k for k in OK if k["id"] == cid)
    x = ec.case_input(c, STORED)
    rng = np.random.default_rng(c["params"]["seed"] + 7000)
    q = rng.normal(0.0, 1e-3, (65, c["n"]))
    if c["dtype"] == "int16":
        batch = np.round(q * 32767.0).astype(np.int16)
    else:
        batch = (np.round(q * 32768.0) / 32768.0).astype(c["dtype"])
    batch[0] = x
    batch[64] = x
    want, want_sync = _oracle_batch(c, batch)
    assert want[0] == c["out"] and want[64] == c["out"]
    pl, got, sync = _run(c, batch, layout)
    print(cid, layout, "->", pl.last_layout(), "lowpass", pl.last_lowpass(), "exact", pl.exact_streams())
    bad = [i for i in range(65) if got[i] != want[i] or sync[i] != want_sync[i]]
    assert not bad, (cid, layout, bad)
    assert pl.last_layout() == layout
