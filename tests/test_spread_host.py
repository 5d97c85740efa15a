"""spread without a GPU: the numpy restatement in
tests/spread_cases.py (the checker of the GPU kernels) is itself a working
modem -- it recovers its own frames, aligned, from random delays to the sample,
and under noise as loud as the signal --, its rules are total, the geometry's
limits are refused on the host, and the C ABI refuses bad arguments before any
device work."""
import ctypes

import numpy as np
import pytest

import ofdm_cases as oc
import spread_cases as sp

NOISY = [(9600, 12000.0), (19200, 24000.0)]
TRIALS = 12
# seeds of test_noise_as_loud_as_the_signal whose capture decodes without acquisition all the same (on the
# restatement): at 19200 chips/s seed 10 is delayed by 1 sample of 80.  Every other seed fails unacquired.
UNACQUIRED_OK = {9600: set(), 19200: {10}}


@pytest.fixture(scope="module")
def product(built_lib):
    """The restatement is only worth testing beside the product it restates."""
    import _amr
    import modem
    for name in ("spread_modulate", "spread_demodulate", "spread_demodulate_batch", "spread_demodulate_soft",
                 "spread_demodulate_soft_batch", "spread_acquire", "spread_acquire_batch"):
        assert callable(getattr(modem, name)), name
    for name in ("dsss_geometry", "design_dsss", "DsssPlan", "get_dsss_plan"):
        assert callable(getattr(_amr, name)), name
    assert _amr.DSSS_CODE == [1, 0, 0, 0, 1, 0, 1, 1, 0, 1, 1, 0, 0, 0, 1, 1]
    assert _amr.TD_SLOTS == ["despread", "slice", "sync_pack", "launch", "acquire"]
    return _amr.lib()


def payload(rng, n):
    return b"FBPC" + rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def recovered(data, sync, msg):
    """The sync word was found and the payload follows it (what lies behind it is the tail's zeros)."""
    return sync >= 0 and data[:len(msg)] == msg


def codes():
    return [(None, b, c) for b, c in oc.CONFIGS] + [(sp.CODE13, 9600, 12000.0), (sp.code64(), 9600, 12000.0)]


def test_the_default_code_has_the_stated_properties(product):
    """DESIGN §3l's criterion: balanced, no cyclic run longer than 3, every off-peak even and odd periodic
    autocorrelation within 4 of 16, and the smallest such 16-bit word with a leading 1."""
    import _amr

    def good(word):
        c = np.array([(word >> (15 - i)) & 1 for i in range(16)])
        if c.sum() != 8:
            return False
        cc = np.concatenate([c, c])
        if any(len(set(cc[i:i + 4])) == 1 for i in range(16)):
            return False
        s = 1 - 2 * c
        for k in range(1, 16):
            head, tail = int(np.dot(s[:16 - k], s[k:])), int(np.dot(s[16 - k:], s[:k]))
            if abs(head + tail) > 4 or abs(head - tail) > 4:
                return False
        return True

    word = int("".join(map(str, _amr.DSSS_CODE)), 2)
    assert word == 0x8B63 and good(word)
    assert not any(good(w) for w in range(0x8000, word))


@pytest.mark.parametrize("code,baud,carrier", codes())
def test_aligned_and_delayed_round_trips(product, code, baud, carrier):
    """The aligned clean capture comes back exactly, sync at bit 80; from random delays below 3 L, digital
    silence before and 2 L after, a clean capture gives o == t % L exactly and its payload."""
    rng = np.random.default_rng(int(baud) + (0 if code is None else len(code)))
    spc, L, cyc, c = sp.geometry(baud, carrier, code)
    assert L == c.size * spc and 1 <= cyc and 2 * cyc < L
    msg = payload(rng, int(rng.integers(20, 61)))
    w = sp.modulate(msg, baud, carrier, code)
    assert w.dtype == np.float32 and w.size == (81 + 8 * len(msg)) * L
    data, sync, o = sp.demod(w, baud, carrier, code, acquire_=False)
    assert (data, sync, o) == (msg, sp.SYNC_AT, 0)
    sdata, soft, ssync, _ = sp.demod_soft(w, baud, carrier, code, acquire_=False)
    assert (sdata, ssync) == (data, sync) and np.packbits(soft > 0).tobytes() == data
    assert np.all(np.abs(soft.astype(int)) >= 126)           # a clean capture: every product on the real axis
    for _ in range(3):
        t = int(rng.integers(0, 3 * L))
        x = sp.delayed(msg, t, baud, carrier, code)
        assert x.size == t + w.size + 2 * L
        o, P = sp.acquire(x, baud, carrier, code)
        assert P.shape == (L,) and o == t % L, (t, o)
        data, sync, o2 = sp.demod(x, baud, carrier, code)
        assert o2 == o and recovered(data, sync, msg) and sync == sp.SYNC_AT + t // L


@pytest.mark.parametrize("baud,carrier", NOISY)
def test_noise_as_loud_as_the_signal(product, baud, carrier):
    """N(0, 1.0^2) on a sine of amplitude 1, about -3 dB per sample: every one of the 12 seeded captures, delayed
    at random, gives its payload back with o within one sample of the delay, circularly.  Scan on the
    restatement (12 seeds each): sigma 1.0 -> 12 of 12 at 9600 chips/s and 12 of 12 at 19200 chips/s, every o
    exact; no lower sigma was needed.  Unacquired, the same captures fail except where UNACQUIRED_OK says."""
    spc, L, cyc, c = sp.geometry(baud, carrier)
    for seed in range(TRIALS):
        rng = np.random.default_rng(1000 * seed + int(baud))
        msg = payload(rng, int(rng.integers(20, 61)))
        t = int(rng.integers(0, 3 * L))
        x = sp.delayed(msg, t, baud, carrier, sigma=1.0, rng=rng)
        data, sync, o = sp.demod(x, baud, carrier)
        assert recovered(data, sync, msg), (seed, t, o)
        assert min((o - t) % L, (t - o) % L) <= 1, (seed, t, o)
        plain = sp.demod(x, baud, carrier, acquire_=False)
        assert recovered(*plain[:2], msg) == (seed in UNACQUIRED_OK[baud]), seed


def test_invalid_geometries(product):
    import _amr
    import modem
    g = _amr.dsss_geometry
    assert g(9600, 12000.0)[:3] == (10, 160, 20)
    assert g(9600, 12000.0, [0, 1])[:3] == (10, 20, 3) and g(9600, 12000.0, [1] * 64)[1] == 640
    bad = [
        dict(code=[1]), dict(code=[0, 1] * 32 + [1]),                      # C of 1 and 65
        dict(code=[0, 1, 2, 1]),                                           # a code entry of 2
        dict(carrier=100.0),                                               # cyc = floor(100 * 160 / 96000 + 0.5) = 0
        dict(carrier=48000.0), dict(carrier=47900.0),                      # 2 cyc >= L
        dict(baud=200000),                                                 # spc = 0
    ]
    for kw in bad:
        args = dict(baud=9600, carrier=12000.0, code=None)
        args.update(kw)
        with pytest.raises(ValueError):
            g(args["baud"], args["carrier"], args["code"])
        with pytest.raises(ValueError):                      # before any device work: no GPU is needed to refuse
            modem.spread_demodulate(np.zeros(4000, np.float32), args["baud"], args["carrier"], args["code"])
        with pytest.raises(ValueError):
            modem.spread_modulate(b"x", args["baud"], args["carrier"], args["code"])
        with pytest.raises(ValueError):
            modem.spread_acquire_batch(np.zeros((0, 10), np.float32), args["baud"], args["carrier"], args["code"])
    assert g(9600, 47000.0)[2] == 78 and g(9600, 47600.0)[2] == 79       # 2 * 79 < 160: the highest valid cyc
    # the C side refuses the same before any device work
    L = product
    h = ctypes.c_void_p()
    spc, Lb, cyc, c, Wc, T, Sn, cs = _amr.design_dsss(9600, 12000.0)
    p = _amr.ptr
    inv = _amr.AMR_E_INVALID
    create = L.amr_dsss_plan_create
    assert create(ctypes.byref(h), 0, 1000, 10, 1, 20, p(Wc), p(T), p(cs), 1) == inv
    assert create(ctypes.byref(h), 0, 1000, 10, 65, 20, p(Wc), p(T), p(cs), 1) == inv
    assert create(ctypes.byref(h), 0, 1000, 0, 16, 20, p(Wc), p(T), p(cs), 1) == inv
    assert create(ctypes.byref(h), 0, 1000, 10, 16, 0, p(Wc), p(T), p(cs), 1) == inv
    assert create(ctypes.byref(h), 0, 1000, 10, 16, 80, p(Wc), p(T), p(cs), 1) == inv
    assert create(ctypes.byref(h), 0, 1000, 1 << 21, 16, 20, p(Wc), p(T), p(cs), 1) == inv   # L > 2^24
    assert create(ctypes.byref(h), 0, -1, 10, 16, 20, p(Wc), p(T), p(cs), 1) == inv
    assert create(ctypes.byref(h), 0, 1000, 10, 16, 20, p(Wc), p(T), p(cs), 0) == inv
    assert create(ctypes.byref(h), 0, 1000, 10, 16, 20, None, p(T), p(cs), 1) == inv
    two = cs.copy()
    two[3] = -3.0                                            # what a code entry of 2 becomes
    assert create(ctypes.byref(h), 0, 1000, 10, 16, 20, p(Wc), p(T), p(two), 1) == inv
    assert b"chip sign" in L.amr_last_error()


def test_the_bit_rule_and_the_soft_signs_are_total(product):
    nan, inf = np.nan, np.inf
    vals = [0.0, -0.0, 1.0, -1.0, 2.0 ** 500, -2.0 ** 500, 2.0 ** -500, -2.0 ** -500, 5e-324, -5e-324, inf, -inf, nan]
    d = np.array([complex(a, b) for a in vals for b in vals])
    bits = sp.bits_of_products(d)
    assert bits.dtype == np.uint8 and set(bits.tolist()) == {0, 1}
    assert np.array_equal(bits == 1, np.array([a < 0 for a in vals for _ in vals]))
    assert bits[np.isnan(d.real)].sum() == 0 and bits[d.real == 0].sum() == 0
    # through the product model: symbols of every scale, the soft sign is the hard bit wherever both are defined
    rng = np.random.default_rng(4)
    for scale in (1.0, 2.0 ** 500, 2.0 ** -500, 2.0 ** -530):
        Y = (rng.standard_normal(200) + 1j * rng.standard_normal(200)) * scale
        Y[7] = 0.0
        Y[50] = complex(nan, 1.0)
        Y[90] = complex(inf, -inf)
        b, s = sp.slice_bits(Y), sp.soft(Y)
        assert b.shape == s.shape == (199,) and np.array_equal(s > 0, b == 1)
        assert np.all((np.abs(s.astype(int)) >= 1) & (np.abs(s.astype(int)) <= 127))
        assert b[6] == b[7] == 0 and s[6] == s[7] == -1      # a zero symbol: the product is zero, the bit 0, magnitude 1
        assert b[49] == b[50] == 0                           # a NaN component: 0
    assert sp.slice_bits(np.zeros(1, np.complex128)).size == 0 and sp.soft(np.zeros(0, np.complex128)).size == 0
    # first_max
    fm = sp.first_max
    assert fm(np.array([nan, 1.0, 2.0])) == 0                # a NaN P[0] keeps 0
    assert fm(np.array([1.0, nan, 2.0, nan, 2.0])) == 2      # NaN elsewhere never wins; the first maximum
    assert fm(np.array([0.0, 0.0, 0.0])) == 0 and fm(np.array([3.0])) == 0
    assert fm(np.array([1.0, inf, inf])) == 1 and fm(np.array([-0.0, 0.0])) == 0


def test_shift_and_short_captures(product):
    x = np.arange(1, 6, dtype=np.float32)
    assert sp.shift(x, 0).tolist() == [1, 2, 3, 4, 5] and sp.shift(x, 2).tolist() == [3, 4, 5, 0, 0]
    assert sp.shift(x, 4).tolist() == [5, 0, 0, 0, 0] and sp.shift(x, 5).tolist() == [0] * 5
    assert sp.shift(x, 1).dtype == np.float32 and sp.shift(np.zeros(0), 0).size == 0
    baud, carrier = 9600, 12000.0
    L = 160
    for n in (0, 1, L - 1, L, 2 * L - 2):                    # M = 0: nothing to acquire, o = 0
        o, P = sp.acquire(np.ones(n, np.float32), baud, carrier)
        assert o == 0 and not P.any() and sp.acq_bits(n, L) == 0
    assert sp.acq_bits(2 * L - 1, L) == 1 and sp.acq_bits(3 * L - 2, L) == 1 and sp.acq_bits(3 * L - 1, L) == 2
    for n in (0, L, 2 * L - 1):                              # S < 2: b"", sync -1
        assert sp.demod(np.ones(n, np.float32), baud, carrier)[:2] == (b"", -1)
        assert sp.demod_soft(np.ones(n, np.float32), baud, carrier, acquire_=False)[0] == b""
    # all-zero input: every P is 0.0, nothing is above P[0]
    o, P = sp.acquire(np.zeros(1000, np.float32), baud, carrier)
    assert o == 0 and not P.any()
    # a NaN at sample 0 enters P[0] (and its neighbours): 0 is kept; a NaN elsewhere never wins
    rng = np.random.default_rng(9)
    msg = payload(rng, 20)
    x = sp.delayed(msg, 77, baud, carrier)
    x[0] = np.nan
    o, P = sp.acquire(x, baud, carrier)
    assert np.isnan(P[0]) and o == 0
    x[0] = 0.0
    # every sample below M L lies in one window of every offset; sample M L + 100 only in those of d >= 101
    k = sp.acq_bits(x.size, L) * L + 100
    assert k < x.size
    x[k] = np.nan
    o, P = sp.acquire(x, baud, carrier)
    assert np.flatnonzero(np.isnan(P)).tolist() == list(range(101, L)) and o == 77


def test_segment_order_is_part_of_the_definition(product):
    """More than one segment: P is the sum of the segments' sums, not one running sum."""
    rng = np.random.default_rng(2)
    baud, carrier, fs, code = 1000, 1250.0, 5000, [1, 0, 0]  # spc 5, L 15
    spc, L, cyc, c, Wc, T, Sn, cs = __import__("_amr").design_dsss(baud, carrier, code, fs)
    assert (spc, L) == (5, 15)
    x = rng.standard_normal(131 * L - 1)
    assert sp.acq_bits(x.size, L) == 130
    P = sp.energy(x, baud, carrier, code, fs)
    ur, ui = sp.chip_sums(x, baud, carrier, code, fs)
    d = np.arange(L)
    run, parts = np.zeros(L), []
    for s in range(130):
        yr, yi = np.zeros(L), np.zeros(L)
        for j in range(3):
            yr = yr + cs[j] * ur[d + s * L + j * spc]
            yi = yi + cs[j] * ui[d + s * L + j * spc]
        run = run + (yr * yr + yi * yi)
        if s % 64 == 63 or s == 129:
            parts.append(run)
            run = np.zeros(L)
    assert len(parts) == 3 and np.array_equal(P, (parts[0] + parts[1]) + parts[2])


def test_entry_argument_checks(product):
    import _amr
    import modem
    L = product
    inv = _amr.AMR_E_INVALID
    p = _amr.ptr
    x = np.zeros((1, 400), np.float32)
    out = np.zeros((1, 64), np.uint8)
    ln, sy, of = (np.zeros(1, np.int64) for _ in range(3))
    soft = np.zeros((1, 512), np.int8)
    P = np.zeros((1, 160))
    Y = np.zeros((1, 5, 2))
    words = np.zeros((1, 1), np.uint32)
    assert L.amr_dsss_demod_host(None, p(x), 0, 1, 400, p(out), 64, p(ln), p(sy), p(soft), 512, p(of), 1) == inv
    assert b"amr_dsss_demod_host" in L.amr_last_error()
    assert L.amr_dsss_demod_device(None, p(x), 0, 1, 400, p(out), 64, p(ln), p(sy), None, 0, None, 0) == inv
    assert L.amr_dsss_demod_host(None, p(x), 0, -1, 400, p(out), 64, p(ln), p(sy), None, 0, None, 1) == inv
    assert b"negative" in L.amr_last_error()
    assert L.amr_dsss_acquire_host(None, p(x), 0, 1, 400, p(of), p(P)) == inv
    assert b"amr_dsss_acquire_host" in L.amr_last_error()
    assert L.amr_dsss_acquire_device(None, p(x), 0, 1, 400, p(of), None) == inv
    assert L.amr_dsss_symbols_at_host(None, p(x), 0, 1, 400, p(of), p(Y)) == inv
    assert L.amr_dsss_slice_host(p(Y), 1, 5, None) == inv and L.amr_dsss_slice_host(None, 1, 5, p(words)) == inv
    assert L.amr_dsss_soft_host(p(Y), 1, 5, None) == inv and L.amr_dsss_soft_host(p(Y), -1, 5, p(soft)) == inv
    assert L.amr_dsss_slice_host(None, 0, 0, None) == _amr.AMR_OK and L.amr_dsss_soft_host(p(Y), 1, 1, p(soft)) == _amr.AMR_OK
    assert L.amr_dsss_plan_out_capacity(None) == -1 and L.amr_dsss_plan_scratch_bytes(None) == -1
    assert L.amr_dsss_plan_synchronize(None) == inv and L.amr_dsss_plan_enable_timing(None, 1) == inv
    assert L.amr_dsss_plan_timings(None, None, 5) == inv and L.amr_dsss_plan_destroy(None) == _amr.AMR_OK
    # the modulator's checks
    spc, Lb, cyc, c, Wc, T, Sn, cs = _amr.design_dsss(9600, 12000.0)
    nb = np.array([3], np.int64)
    data = np.zeros((1, 3), np.uint8)
    o32 = np.zeros((1, 100), np.float32)
    mod = L.amr_dsss_modulate_host
    assert mod(10, 16, 20, p(cs), p(Sn), p(data), 3, p(nb), 1, p(o32), 99, 100, None, 0) == inv   # out_stride < n_out
    assert mod(10, 16, 20, None, p(Sn), p(data), 3, p(nb), 1, p(o32), 100, 100, None, 0) == inv
    assert mod(10, 16, 0, p(cs), p(Sn), p(data), 3, p(nb), 1, p(o32), 100, 100, None, 0) == inv
    assert mod(10, 16, 20, p(cs), p(Sn), p(data), 2, p(nb), 1, p(o32), 100, 100, None, 0) == inv  # n_bytes > stride
    assert mod(10, 16, 20, p(cs), p(Sn), None, 0, None, 0, None, 0, 0, None, 0) == _amr.AMR_OK     # empty batch
    # the byte estimates are host arithmetic
    est, acq = L.amr_dsss_plan_bytes_estimate, L.amr_dsss_acquire_bytes_estimate
    assert acq(96000, 10, 16, 1) == (10 * 160 + 160) * 8 + 8               # M = 599: 10 segments
    assert acq(96000, 10, 16, 4096) == 4096 * acq(96000, 10, 16, 1)
    assert acq(300, 10, 16, 2) == 8 + 2 * (160 * 8 + 8)                     # M = 0: no segment
    assert acq(96000, 10, 65, 1) < 0 and acq(96000, 0, 16, 1) < 0 and acq(96000, 10, 16, 0) < 0 and acq(-1, 10, 16, 1) < 0
    e1, e2 = est(96000, 10, 16, 1), est(96000, 10, 16, 64)
    assert 0 < e1 < e2 < 64 * e1 + 1 and est(96000, 10, 1, 1) < 0 and est(96000, 10, 16, 0) < 0
    if _amr.device_count() < 1:
        z = np.zeros(4000, np.float32)
        for call in (lambda: modem.spread_acquire(z, 9600, 12000.0), lambda: modem.spread_demodulate(z, 9600, 12000.0),
                     lambda: modem.spread_demodulate_soft(z, 9600, 12000.0, acquire=False),
                     lambda: modem.spread_modulate(b"FBPC", 9600, 12000.0),
                     lambda: modem.modulate_batch("spread", [b"a"], 9600, 12000.0)):
            with pytest.raises(_amr.AmrError):
                call()
    with pytest.raises(ValueError):
        modem.spread_acquire(np.zeros((2, 4000), np.float32), 9600, 12000.0)
    with pytest.raises(ValueError):
        modem.spread_demodulate(np.zeros((2, 4000), np.float32), 9600, 12000.0)
    assert modem.spread_acquire_batch(np.zeros((0, 100), np.float32), 9600, 12000.0).shape == (0,)
    assert modem.spread_demodulate_batch(np.zeros((0, 100), np.float32), 9600, 12000.0) == []
    assert modem.spread_demodulate_soft_batch(np.zeros((0, 100), np.float32), 9600, 12000.0) == ([], [])


def test_the_alias_is_untouched(product):
    """dsss_modulate stays the reference's BPSK call: same function body, nothing spread."""
    import inspect
    import modem
    assert "bpsk_modulate" in inspect.getsource(modem.dsss_modulate)
