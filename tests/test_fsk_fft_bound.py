"""F2's margin scale tau from a standard FFT rounding bound (VERDICT r5 item
2, FSK half; csrc/fsk_api.cpp fsk_fft_bound).

F2 keeps an envelope compare only when |env_mark - env_space| > 2 tau
peak|ext x|.  The fast path's and pocketfft's envelopes each differ from the
exact |hilbert(z)| by at most (4 eps + 4u) ||z||_2 (eps: the transform's
relative 2-norm error), so tau >= (4 eps_fast + 4 eps_ref + 8u) max ||z||_2 /
peak makes every kept compare the reference's.  Checked here, on the CPU:
  * libamr.so's tau is this formula (restated below) at two-pass, six-step
    and Bluestein lengths, and never below 2^-36;
  * the ||z||_2 bound (both filtfilt passes' L1 gain and zi transients)
    holds for the oracle's band-pass output of real signals;
  * pocketfft's own envelope error (the oracle's float64 restatement vs
    scipy in long double) is below its share of the bound -- printed with
    the ratio.  The fast path's side is measured on the GPU
    (tests/test_gpu_fsk.py::test_envelope_error_is_far_below_the_margin)."""
import math

import numpy as np
import pytest

CASES = [(96000, 9600, 12000.0, 24000.0), (48000, 1200, 2400.0, 4800.0), (960000, 9600, 12000.0, 24000.0),
         (96001, 9600, 12000.0, 24000.0), (24001, 1200, 2400.0, 4800.0), (441000, 2400, 7000.0, 19000.0),
         (30000, 2400, 11229.28, 29833.37)]
U = 2.0 ** -53


def _lpf(n):
    r, q = 1, 2
    while q * q <= n:
        while n % q == 0:
            r, n = q, n // q
        q += 1
    return max(r, n) if n > 1 else r


def _restated(n, d, G, R, pad=21):
    """The bound restated from its definition (fsk_api.cpp fsk_fft_bound)."""
    gam = lambda k: k * U / (1 - k * U)   # noqa: E731

    def eta(p):
        r = max(p, 2)
        return max(8.5 * U, math.sqrt(r) * gam(r + 4.0) / max(1.0, math.log2(r))) + 2 * U

    def eps_direct(M, p):
        e = math.ceil(math.log2(max(M, 2))) * eta(p)
        return e / (1 - e)

    gc = math.sqrt(2) * gam(2.0) + 2 * U

    def eps_blue(M):
        em = eps_direct(M, _lpf(M))
        return (6 + 2 * math.log(n)) * (2 * em + 2 * gc) + math.sqrt(2.0 * n - 1) * em + gc

    ef = eps_blue(d["fast_M"]) if d["fast_blue"] else eps_direct(n, _lpf(n))
    er = eps_blue(d["ref_M"]) if d["ref_blue"] else eps_direct(n, _lpf(d["ref_M"]))
    m1 = n + 2 * pad
    zb = max(g * g * math.sqrt(m1) + 2 * g * r + r * r for g, r in zip(G, R))
    return max(2.0 ** -36, (4 * ef + 4 * er + 8 * U) * zb * (1 + 2.0 ** -20)), ef, er, zb


def _gains(b, a, zi):
    from scipy import signal
    imp = np.zeros(400000)
    imp[0] = 1.0
    G = np.abs(signal.lfilter(b, a, imp)).sum()
    r, _ = signal.lfilter(b, a, np.zeros(400000), zi=zi)
    return G, float(np.sqrt((r * r).sum()))


@pytest.mark.parametrize("n,baud,mark,space", CASES, ids=lambda v: str(v))
def test_tau_is_the_standard_bound(n, baud, mark, space, built_lib):
    import _fsk
    d = _fsk.fft_margin(n, baud, mark, space)
    _, ((mb, ma, mz), (sb, sa, sz)) = _fsk.design_fsk(n, baud, mark, space, 96000.0)
    G, R = zip(*(_gains(b, a, z) for b, a, z in ((mb, ma, mz), (sb, sa, sz))))
    G = [g * (1 + 2.0 ** -20) for g in G]       # the library's safety factors on its response sums
    R = [r * (1 + 2.0 ** -30) for r in R]
    tau, ef, er, zb = _restated(n, d, G, R)
    # the library's gains come from its own response loops (double / long
    # double), so the restatement agrees to the gains' rounding
    assert d["tau"] >= 2.0 ** -36
    assert math.isclose(d["eps_fast"], ef, rel_tol=1e-12) and math.isclose(d["eps_ref"], er, rel_tol=1e-12)
    assert math.isclose(d["zmax"], zb, rel_tol=1e-6), (d["zmax"], zb)
    assert math.isclose(d["tau"], tau, rel_tol=1e-6), (d["tau"], tau)
    print(f"n={n}: tau {d['tau']:.3e} = {d['tau'] / 2.0 ** -36:.1f} x 2^-36 (fast {'Bluestein M=' + str(d['fast_M']) if d['fast_blue'] else 'direct'}, "
          f"pocketfft {'Bluestein M=' + str(d['ref_M']) if d['ref_blue'] else 'direct'})")


@pytest.mark.parametrize("n", [77, 1000, 1001, 24001, 96001])
def test_chirp_spectrum_bound(n):
    """Bluestein's kernel (the chirp exp(i pi m^2 / n), |m| < n, wrapped into
    a length-M >= 2n - 1 transform) has max |FFT_M| <= sqrt(n) (6 + 2 ln n),
    the constant fsk_fft_bound takes (measured: ~2.2 sqrt(n))."""
    M = 1
    while M < 2 * n - 1:
        M *= 2
    for MM in (M, 2 * n - 1 + (n % 7)):
        b = np.zeros(MM, complex)
        k = np.arange(n, dtype=np.float64)
        b[:n] = np.exp(1j * np.pi * ((k * k) % (2 * n)) / n)
        b[MM - n + 1:] = b[1:n][::-1]
        assert np.abs(np.fft.fft(b)).max() <= math.sqrt(n) * (6 + 2 * math.log(n))


@pytest.mark.parametrize("n,baud,mark,space", [CASES[0], CASES[1], CASES[3], CASES[4], CASES[6]],
                         ids=lambda v: str(v))
def test_pocketfft_error_within_its_share(n, baud, mark, space, built_lib):
    """scipy's |hilbert(z)| (the oracle's restatement of pocketfft, bit-exact
    with scipy) vs the same in long double (scipy.fft runs long double
    natively), on the band-pass output of a modulated capture, a noisy one
    and a clipped one: max error <= (4 eps_ref + 4u) ||z||_2, and ||z||_2 <=
    zmax peak|ext x|."""
    import _fsk
    import synth
    from oracle import oracle
    from scipy import signal
    d = _fsk.fft_margin(n, baud, mark, space)
    _, ((mb, ma, _), (sb, sa, _)) = _fsk.design_fsk(n, baud, mark, space, 96000.0)
    rng = np.random.default_rng(n)
    w = synth.fsk_waveform(synth.random_frame(rng, 60), baud, mark, space, 96000.0)
    base = np.zeros(n)
    base[:min(n, w.size)] = w[:n]
    worst_ratio = np.inf
    for x in (base, base + rng.normal(0, 0.3, n), np.clip(3 * base, -1, 1)):
        peak = max(np.abs(x).max(), np.abs(oracle.odd_edges(x, 21)).max())
        for b, a in ((mb, ma), (sb, sa)):
            z = oracle.filtfilt(b, a, x)
            z2 = float(np.sqrt((z * z).sum()))
            assert z2 <= d["zmax"] * peak
            ref = oracle.hilbert_env(z)
            true = np.abs(signal.hilbert(z.astype(np.longdouble)))
            err = float(np.max(np.abs(ref.astype(np.longdouble) - true)))
            share = (4 * d["eps_ref"] + 4 * U) * z2
            assert err <= share, (err, share)
            worst_ratio = min(worst_ratio, share / max(err, 1e-300))
    print(f"n={n}: pocketfft's envelope error <= its bound share / {worst_ratio:.0f}")


def _no_bound_cases():
    """The fixture's parameter sets whose band-pass responses have not decayed
    below 1e-40 within the 4 000 000 steps iir_gains / zi_response_l2 walk
    (csrc/iir_design.h): the slow class, the unstable designs, and a band edge
    1e-6 of Nyquist from 0 or 1."""
    import fsk_edge_cases as ec
    out = [c for c in ec.CASES if c["edge"] in ("slow", "unstable")]
    out += [c for c in ec.CASES if c["id"] in ("e12_edge0", "e15_edge0", "e16_edge0", "e18_edgenyq", "e21_edgenyq")]
    return out


@pytest.mark.parametrize("case", _no_bound_cases(), ids=lambda c: c["id"])
def test_no_bound_for_undecayed_responses(case, built_lib):
    """amr_fsk_fft_margin keeps refusing these (AMR_E_INVALID): there is no
    finite tau to report.  A plan of the same filters is still created -- with
    every stream on the exact path (tests/test_gpu_fsk_edge.py)."""
    import _amr
    import _fsk
    with pytest.raises(_amr.AmrError) as e:
        _fsk.fft_margin(1000, case["baud"], case["f0"], case["f1"], case["samp_rate"])
    assert e.value.code == _amr.AMR_E_INVALID and "no bound" in str(e.value)
