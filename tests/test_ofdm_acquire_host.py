"""ofdm acquisition without a GPU: the numpy restatement in
tests/ofdm_acquire_cases.py (the checker of the GPU kernels) finds the symbol
boundary of a delayed capture, to the sample when it is clean, and the payload
comes back after shift(x, o); the rule is total; and the C ABI refuses bad
arguments before any device work."""
import ctypes

import numpy as np
import pytest

import ofdm_acquire_cases as ac
import ofdm_cases as oc

NOISE = [0.0, 0.05]
KS = [1, 3, 4, 8]


@pytest.fixture(scope="module")
def product(built_lib):
    """The restatement is only worth testing beside the product it restates."""
    import _amr
    import modem
    for name in ("ofdm_acquire", "ofdm_acquire_batch"):
        assert callable(getattr(modem, name)), name
    for name in ("amr_ofdm_acquire_bytes_estimate", "amr_ofdm_acquire_host", "amr_ofdm_acquire_device",
                 "amr_ofdm_symbols_at_host", "amr_ofdm_demod_acq_host", "amr_ofdm_demod_acq_device"):
        assert name in _amr.EXPORTS, name
    assert _amr.TO_SLOTS == _amr.TO_NAMES + ["acquire"]
    return _amr.lib()


def payload(rng, n):
    return b"FBPC" + rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def recovered(data, sync, msg):
    """The sync word was found and the payload follows it (what lies behind it is padding and the tail's zeros)."""
    return sync >= 0 and data[:len(msg)] == msg


@pytest.mark.parametrize("sigma", NOISE)
@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("baud,carrier", oc.CONFIGS)
def test_delayed_capture_round_trip(product, baud, carrier, K, sigma):
    """Every configuration with a cyclic prefix (Ncp >= 1, that is L >= 8) recovers its payload at a random
    delay, and the clean ones find the boundary to the sample.  One of the forty has none: 19200 Bd with K = 1
    is L = 5, Ncp = 0.  There is no prefix to find there, E is all zeros for every input, dhat = 0 and o = 0:
    acquisition changes nothing, and the capture decodes only where the plain receiver decodes it (on the
    restatement, clean: a delay of 0 or 4 mod 5, not 1, 2 or 3; test_no_prefix_means_no_acquisition).  So that
    case asserts what is true of it -- o = dhat = 0 and the plain receiver's bytes -- and not the payload."""
    rng = np.random.default_rng(7 + int(baud) + 100 * K + int(sigma * 100))
    sps, L, Ncp, Nu, bins = oc.geometry(baud, carrier, K)
    msg = payload(rng, int(rng.integers(20, 201)))
    t = int(rng.integers(0, 5 * L))
    x = ac.delayed(msg, t, baud, carrier, K, sigma=sigma, rng=rng)
    assert x.size == t + oc.n_symbols(len(msg), K) * L + L
    o, dhat, E = ac.acquire(x, baud, carrier, K)
    assert E.shape == (L,) and 0 <= dhat < L and -Ncp <= o <= L - 1 - Ncp
    assert o == dhat - Ncp // 2 or o == dhat - Ncp // 2 - L
    data, sync, o2 = ac.demod(x, baud, carrier, K)
    sdata, soft, ssync, o3 = ac.demod_soft(x, baud, carrier, K)
    assert (sdata, ssync, o3) == (data, sync, o) and o2 == o and np.packbits(soft > 0).tobytes() == data
    if Ncp == 0:
        assert (baud, K) == (19200, 1) and (o, dhat) == (0, 0) and not E.any()
        assert (data, sync) == oc.demod(x, baud, carrier, K)
        return
    if not sigma:
        assert (dhat - t) % L == 0, (dhat, t, L)
    assert recovered(data, sync, msg), (baud, K, sigma, t, dhat, o)


def test_no_prefix_means_no_acquisition(product):
    """L < 8 gives Ncp = L // 8 = 0: nothing repeats, so there is nothing to acquire.  o = 0 whatever the delay,
    and a clean capture delayed by 1, 2 or 3 samples of its 5-sample symbol does not decode, with or without
    acquisition; delayed by a whole symbol it does."""
    baud, carrier, K = 19200, 24000.0, 1
    sps, L, Ncp, Nu, bins = oc.geometry(baud, carrier, K)
    assert (L, Ncp) == (5, 0)
    msg = payload(np.random.default_rng(3), 60)
    for t in range(0, 3 * L):
        x = ac.delayed(msg, t, baud, carrier, K)
        data, sync, o = ac.demod(x, baud, carrier, K)
        assert o == 0 and (data, sync) == oc.demod(x, baud, carrier, K)
        if t % L == 0:
            assert recovered(data, sync, msg), t
        if t % L in (1, 2, 3):
            assert not recovered(data, sync, msg), t
    # the smallest symbol that has a prefix: L = 8, Ncp = 1 (12000 Bd, K = 1) is acquired at every delay
    sps, L, Ncp, Nu, bins = oc.geometry(12000, 24000.0, 1)
    assert (L, Ncp) == (8, 1)
    for t in range(0, 2 * L):
        x = ac.delayed(msg, t, 12000, 24000.0, 1)
        o, dhat, _ = ac.acquire(x, 12000, 24000.0, 1)
        assert dhat == t % L and recovered(*ac.demod(x, 12000, 24000.0, 1)[:2], msg), t


@pytest.mark.parametrize("K", [16, 64])
@pytest.mark.parametrize("baud,carrier", oc.CONFIGS)
def test_many_subcarriers_clean(product, baud, carrier, K):
    """Amplitude is 1 / K per subcarrier: K = 16 and 64 are pinned clean only, at every configuration."""
    rng = np.random.default_rng(int(baud) + K)
    sps, L, Ncp, Nu, bins = oc.geometry(baud, carrier, K)
    assert Ncp >= 10
    msg = payload(rng, 150)
    t = int(rng.integers(0, 5 * L))
    x = ac.delayed(msg, t, baud, carrier, K)
    o, dhat, _ = ac.acquire(x, baud, carrier, K)
    assert (dhat - t) % L == 0
    data, sync, _ = ac.demod(x, baud, carrier, K)
    assert recovered(data, sync, msg)


@pytest.mark.parametrize("K", [3, 8])
def test_aligned_capture_decodes_as_today(product, K):
    baud, carrier = 9600, 12000.0
    rng = np.random.default_rng(50 + K)
    sps, L, Ncp, Nu, bins = oc.geometry(baud, carrier, K)
    msg = payload(rng, 90)
    x = ac.delayed(msg, 0, baud, carrier, K)
    o, dhat, _ = ac.acquire(x, baud, carrier, K)
    assert dhat == 0 and o == -(Ncp // 2)
    assert ac.demod(x, baud, carrier, K)[:2] == oc.demod(x, baud, carrier, K)


@pytest.mark.parametrize("K", [3, 8])
def test_delays_just_below_a_symbol_keep_the_first_symbol(product, K):
    """t = L - 1, L - 2, ...: dhat near L gives a negative o, zeros in front instead of a lost reference symbol."""
    baud, carrier = 9600, 12000.0
    rng = np.random.default_rng(60 + K)
    sps, L, Ncp, Nu, bins = oc.geometry(baud, carrier, K)
    msg = payload(rng, 40)
    neg = 0
    for back in range(1, Ncp + 3):
        t = L - back
        x = ac.delayed(msg, t, baud, carrier, K)
        o, dhat, _ = ac.acquire(x, baud, carrier, K)
        assert dhat == t
        assert o == (t - Ncp // 2 if t - Ncp // 2 <= L - 1 - Ncp else t - Ncp // 2 - L)
        data, sync, _ = ac.demod(x, baud, carrier, K)
        assert recovered(data, sync, msg), (K, t, o)
        f = t - o                                # where the frame starts in shift(x, o): half a prefix into a symbol
        assert f % L == Ncp // 2 and sync == oc.SYNC_AT + 2 * K * (f // L)
        neg += o < 0
    assert neg == Ncp - Ncp // 2 and back_off_range(L, Ncp)       # t - Ncp // 2 > L - 1 - Ncp


def back_off_range(L, Ncp):
    os_ = [ac.back_off(d, L, Ncp) for d in range(L)]
    return min(os_) >= -Ncp and max(os_) <= L - 1 - Ncp and len(set(os_)) == L


def test_long_capture_amid_digital_silence(product):
    baud, carrier, K = 9600, 12000.0, 8
    rng = np.random.default_rng(96)
    L = oc.geometry(baud, carrier, K)[1]
    msg = payload(rng, 200)
    w = oc.modulate(msg, baud, carrier, K)
    t = 41237
    x = np.zeros(96000, np.float32)
    x[t:t + w.size] = w
    o, dhat, _ = ac.acquire(x, baud, carrier, K)
    assert dhat == t % L
    data, sync, _ = ac.demod(x, baud, carrier, K)
    assert sync >= 0 and data[:len(msg)] == msg


def test_shift_edges(product):
    x = np.arange(1, 6, dtype=np.float32)
    assert ac.shift(x, 0).tolist() == [1, 2, 3, 4, 5]
    assert ac.shift(x, 2).tolist() == [3, 4, 5, 0, 0]
    assert ac.shift(x, -2).tolist() == [0, 0, 1, 2, 3]
    assert ac.shift(x, 5).tolist() == [0] * 5 and ac.shift(x, -5).tolist() == [0] * 5
    assert ac.shift(x, 9).tolist() == [0] * 5 and ac.shift(x, -9).tolist() == [0] * 5
    assert ac.shift(x, 4).tolist() == [5, 0, 0, 0, 0] and ac.shift(x, -4).tolist() == [0, 0, 0, 0, 1]
    assert ac.shift(x, 1).dtype == np.float32 and ac.shift(np.zeros(0), 3).size == 0
    xi = np.array([7, -8, 9], np.int16)
    assert ac.shift(xi, -1).tolist() == [0, 7, -8] and ac.shift(xi, -1).dtype == np.int16


def test_the_rule_is_total(product):
    nan = np.nan
    # all-zero input: every E is 0.0, nothing is below E[0]
    baud, carrier, K = 9600, 12000.0, 8
    sps, L, Ncp, Nu, bins = oc.geometry(baud, carrier, K)
    o, dhat, E = ac.acquire(np.zeros(1000, np.float32), baud, carrier, K)
    assert dhat == 0 and o == -(Ncp // 2) and not E.any()
    # a single non-zero sample: G is non-zero at two r, E is zero wherever the window misses both: the first of them
    x = np.zeros(1000, np.float32)
    x[3 * L + 5] = 0.5
    G = ac.fold(x, L, Nu)
    assert np.flatnonzero(G).tolist() == [5, 15] and (L, Nu, Ncp) == (80, 70, 10)       # 15 = (5 - Nu) % L
    o, dhat, E = ac.acquire(x, baud, carrier, K)
    zeros = np.flatnonzero(E == 0.0)
    assert E[0] != 0.0 and dhat == zeros[0] == 16 and zeros.size > 1 and o == 11
    # on E directly
    assert ac.first_min(np.array([nan, 1.0, 0.0])) == 0            # a NaN E[0] keeps 0
    assert ac.first_min(np.array([2.0, nan, 1.0, nan, 1.0])) == 2  # NaN elsewhere never wins; the first minimum
    assert ac.first_min(np.array([nan, nan])) == 0
    assert ac.first_min(np.array([1.0, nan, nan])) == 0
    assert ac.first_min(np.array([np.inf, np.inf, np.inf])) == 0
    assert ac.first_min(np.array([np.inf, 3.0, 3.0])) == 1
    assert ac.first_min(np.array([0.0, -0.0, 0.0])) == 0
    assert ac.first_min(np.array([5.0])) == 0
    # a NaN sample poisons the G it enters, and through them the E whose window holds one
    x = np.ones(1000, np.float32)
    x[::3] = 0.25
    clean = ac.acquire(x, baud, carrier, K)
    x[37] = nan                                  # G[37] alone: E[28 .. 37]
    o, dhat, E = ac.acquire(x, baud, carrier, K)
    assert np.flatnonzero(np.isnan(E)).tolist() == list(range(28, 38)) and not np.isnan(E[0])
    keep = ~np.isnan(E)
    assert np.array_equal(E[keep], clean[2][keep]) and dhat == int(np.flatnonzero(E == E[keep].min())[0])
    x[37] = 1.0
    x[5] = nan                                   # G[5]: E[0 .. 5] and, around the end, E[76 .. 79]
    o, dhat, E = ac.acquire(x, baud, carrier, K)
    assert np.flatnonzero(np.isnan(E)).tolist() == list(range(6)) + list(range(76, 80)) and dhat == 0
    # M = 0: fewer samples than Nu + L
    for n in (0, 1, Nu + L - 1):
        assert ac.periods(n, L, Nu) == 0
        o, dhat, E = ac.acquire(np.ones(n, np.float32), baud, carrier, K)
        assert dhat == 0 and o == -(Ncp // 2) and not E.any()
    assert ac.periods(Nu + L, L, Nu) == 1 and ac.periods(Nu + 2 * L - 1, L, Nu) == 1 and ac.periods(Nu + 2 * L, L, Nu) == 2
    # Ncp = 0 (19200 Bd, K = 1: L = 5): E is all zeros whatever the samples
    sps, L, Ncp, Nu, bins = oc.geometry(19200, 24000.0, 1)
    assert (L, Ncp) == (5, 0)
    rng = np.random.default_rng(1)
    o, dhat, E = ac.acquire(rng.standard_normal(200), 19200, 24000.0, 1)
    assert (o, dhat) == (0, 0) and not E.any()
    msg = payload(rng, 30)
    x = ac.delayed(msg, 0, 19200, 24000.0, 1)
    assert ac.demod(x, 19200, 24000.0, 1)[:2] == oc.demod(x, 19200, 24000.0, 1)


def test_segment_order_is_part_of_the_definition(product):
    """More than one segment: G is the sum of the segments' sums, not one running sum."""
    rng = np.random.default_rng(2)
    L, Nu = 15, 14
    x = rng.standard_normal(130 * L + Nu)
    assert ac.periods(x.size, L, Nu) == 130
    G = ac.fold(x, L, Nu)
    run = np.zeros(L)
    parts = []
    for s in range(130):
        d = x[s * L:s * L + L] - x[s * L + Nu:s * L + Nu + L]
        run = run + d * d
        if s % 64 == 63 or s == 129:
            parts.append(run)
            run = np.zeros(L)
    assert len(parts) == 3 and np.array_equal(G, (parts[0] + parts[1]) + parts[2])


def test_entry_argument_checks(product):
    import _amr
    L = product
    inv = _amr.AMR_E_INVALID
    p = _amr.ptr
    x = np.zeros((1, 400), np.float32)
    out = np.zeros((1, 64), np.uint8)
    ln, sy, of, dh = (np.zeros(1, np.int64) for _ in range(4))
    soft = np.zeros((1, 512), np.int8)
    E = np.zeros((1, 80))
    Y = np.zeros((1, 5, 8, 2))
    assert L.amr_ofdm_acquire_host(None, p(x), 0, 1, 400, p(of), p(dh), p(E)) == inv
    assert b"amr_ofdm_acquire_host" in L.amr_last_error()
    assert L.amr_ofdm_acquire_device(None, p(x), 0, 1, 400, p(of), None, None) == inv
    assert L.amr_ofdm_symbols_at_host(None, p(x), 0, 1, 400, p(of), p(Y)) == inv
    assert L.amr_ofdm_demod_acq_host(None, p(x), 0, 1, 400, p(out), 64, p(ln), p(sy), p(soft), 512, p(of)) == inv
    assert L.amr_ofdm_demod_acq_device(None, p(x), 0, 1, 400, p(out), 64, p(ln), p(sy), None, 0, None) == inv
    assert L.amr_ofdm_demod_acq_host(None, p(x), 0, -1, 400, p(out), 64, p(ln), p(sy), None, 0, None) == inv
    assert b"negative" in L.amr_last_error()
    # the byte estimate is host arithmetic: segments x L + 2 L doubles and two int64 per stream
    est = L.amr_ofdm_acquire_bytes_estimate
    assert est(96000, 10, 8, 1) == (19 * 80 + 2 * 80) * 8 + 16              # M = 1199: 19 segments
    assert est(96000, 10, 8, 4096) == 4096 * est(96000, 10, 8, 1)
    assert est(100, 10, 8, 2) == 8 + 2 * (2 * 80 * 8 + 16)                   # M = 0: no segment
    assert est(96000, 10, 65, 1) < 0 and est(96000, 0, 8, 1) < 0 and est(96000, 10, 8, 0) < 0
    assert est(-1, 10, 8, 1) < 0
    if _amr.device_count() < 1:
        import modem
        with pytest.raises(_amr.AmrError):
            modem.ofdm_acquire(np.zeros(4000, np.float32), 9600, 12000.0, 8)
        with pytest.raises(_amr.AmrError):
            modem.ofdm_demodulate(np.zeros(4000, np.float32), 9600, 12000.0, 8, acquire=True)
    import modem
    with pytest.raises(ValueError):
        modem.ofdm_acquire(np.zeros(4000, np.float32), 9600, 12000.0, 65)
    with pytest.raises(ValueError):
        modem.ofdm_acquire(np.zeros((2, 4000), np.float32), 9600, 12000.0, 8)
    assert modem.ofdm_acquire_batch(np.zeros((0, 100), np.float32), 9600, 12000.0, 8).shape == (0,)
