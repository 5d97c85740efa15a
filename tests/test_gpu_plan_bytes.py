"""The byte totals a plan reports, step by step through every path that
allocates: amr_psk_plan_scratch_bytes, amr_fsk_plan_scratch_bytes,
amr_fsk_plan_resident_bytes and both *_bytes_estimate entries are sums over
the plan's device buffers, and a change to how the host layer owns those
buffers must not move any of them by a byte.

Shape: n = 24000 at 9600 baud with max_streams = 3, the smallest at which the
split and strict paths of both modems run (test_gpu_split.py
test_explicit_chunk_after_a_strict_call).

The constants below were recorded by running these same sequences
(psk_steps / fsk_steps) against the library built from the commit before the
buffers got a single owner (6c6401c, hand-kept byte counters), on an MI355X;
they are not taken from the code they now check.
"""
import numpy as np
import pytest

from _util import fsk_device_demod

pytestmark = pytest.mark.gpu

N, BAUD, FS, B = 24000, 9600, 96000, 3
FC, MARK, SPACE = 3000.0, 12000.0, 24000.0

# (step, (scratch_bytes, bytes_estimate))
PSK_WANT = [
    ("create", (51188396, 51188396)),
    ("split strict B=1", (51188396, 51188396)),
    ("split strict B=3", (51188396, 51188396)),
    ("split_bounds", (51188396, 51188396)),
    ("split_symbols 130", (51188396, 51188396)),
    ("demod_host_raw", (51188396, 51188396)),
    ("row B=3", (51188396, 51188396)),
    ("lane B=3", (51188396, 51188396)),
]
# (step, (scratch_bytes, resident_bytes, bytes_estimate))
FSK_WANT = [
    ("create", (13499815, 9821704, 13499815)),
    ("device entry", (13499815, 11539576, 13499815)),
    ("demod_host B=1", (13499815, 12232735, 13499815)),
    ("demod_host B=3", (13499815, 12232735, 13499815)),
    ("split_bounds", (13499815, 12232735, 13499815)),
    ("split_bandpass 130", (13499815, 12232735, 13499815)),
    ("demod_host_raw", (13499815, 12232735, 13499815)),
    ("envelopes", (13499815, 12232735, 13499815)),
]


@pytest.fixture(scope="module", autouse=True)
def gpu(built_lib):
    import _amr
    if _amr.device_count() < 1:
        pytest.fail("no GPU visible: -m gpu tests must run on the MI355X")


def _raw16(x):
    return np.round(np.clip(x, -1, 1) * 32767).astype(np.int16)


def psk_steps():
    """Yield (step, bytes tuple) after each call of the PSK sequence; every
    decoding step's bytes are checked against the oracle on the way."""
    import _amr
    import synth
    from oracle import oracle
    x = synth.qpsk_batch(B, N, BAUD, carrier=FC, samp_rate=FS, seed=5, distinct=B, noise=0.2)
    xr = _raw16(x)
    want = oracle.psk_demod_batch("qpsk", x, BAUD, FC, FS)[0]
    want_raw = oracle.psk_demod_batch("qpsk", xr, BAUD, FC, FS, raw_int16=True)[0]
    pl = _amr.PskPlan("qpsk", N, BAUD, FC, FS, max_streams=B)
    est = int(_amr.lib().amr_psk_plan_bytes_estimate(_amr.PSK_QPSK, N, pl.sps, pl.first, 9, 5, B))

    def state():
        return pl.scratch_bytes(), est

    yield "create", state()
    pl.set_layout("split")
    pl.set_split_strict(True)
    got, _ = pl.demod_host(x[:1])
    assert pl.last_layout() == "split" and pl.last_strict() and list(got) == list(want[:1])
    yield "split strict B=1", state()
    got, _ = pl.demod_host(x)
    assert pl.last_strict() and list(got) == list(want)
    yield "split strict B=3", state()
    pl.split_bounds(x)
    yield "split_bounds", state()
    pl.split_symbols(x, 130)
    assert pl.split_info()["chunk"] == 130
    yield "split_symbols 130", state()
    got, _ = pl.demod_host_raw(xr)
    assert list(got) == list(want_raw)
    yield "demod_host_raw", state()
    pl.set_layout("row")
    got, _ = pl.demod_host(x)
    assert pl.last_layout() == "row" and list(got) == list(want)
    yield "row B=3", state()
    pl.set_layout("lane")
    got, _ = pl.demod_host(x)
    assert pl.last_layout() == "lane" and list(got) == list(want)
    yield "lane B=3", state()


def fsk_steps():
    """The FSK sequence: (step, bytes tuple) after each call."""
    import _amr
    import _fsk
    import synth
    from oracle import oracle
    x = synth.fsk_batch(B, N, BAUD, MARK, SPACE, seed=9, distinct=B, noise=0.2)
    xr = _raw16(x)
    want = [oracle.fsk_demodulate(r, BAUD, MARK, SPACE) for r in x]
    want_raw = [oracle.fsk_demodulate(r, BAUD, MARK, SPACE, raw_int16=True) for r in xr]
    pl = _fsk.FskPlan(N, BAUD, MARK, SPACE, max_streams=B)
    est = int(_amr.lib().amr_fsk_plan_bytes_estimate(N, pl.sps, 7, B))

    def state():
        return pl.scratch_bytes(), pl.resident_bytes(), est

    yield "create", state()
    got, _ = fsk_device_demod(pl, x)
    assert got == want
    yield "device entry", state()
    got, _ = pl.demod_host(x[:1])
    assert got == want[:1]
    yield "demod_host B=1", state()
    got, _ = pl.demod_host(x)
    assert got == want
    yield "demod_host B=3", state()
    pl.split_bounds(x)
    yield "split_bounds", state()
    pl.split_bandpass(x, 130)
    assert pl.split_info()["chunk"] == 130
    yield "split_bandpass 130", state()
    got, _ = pl.demod_host_raw(xr)
    assert got == want_raw
    yield "demod_host_raw", state()
    m, s = pl.envelopes(x)
    assert np.isfinite(m).all() and np.isfinite(s).all()
    yield "envelopes", state()


def test_psk_plan_bytes_step_by_step():
    got = list(psk_steps())
    print(got)
    assert all(t[0] == t[1] for _, t in got), got          # estimate == scratch_bytes() throughout
    assert got == PSK_WANT


def test_fsk_plan_bytes_step_by_step():
    got = list(fsk_steps())
    print(got)
    assert all(t[0] == t[2] for _, t in got), got          # estimate == scratch_bytes() throughout
    assert got == FSK_WANT
