"""minshift without a GPU: the numpy restatement in
tests/minshift_cases.py (the checker of the GPU kernels) is itself a working
modem -- it recovers its own frames, aligned, from random delays to the sample,
at every valid geometry of up to 12 samples per bit, and under noise --, its
rules are total, the geometry's limits are refused on the host, and the C ABI
refuses bad arguments before any device work."""
import ctypes

import numpy as np
import pytest

import minshift_cases as mc
import ofdm_cases as oc

TRIALS = 12
# test_noise: per (baud, carrier) the largest sigma of the ladder 0.2, 0.3 .. 1.2 at which the restatement
# returns every one of the 12 seeded payloads with o within L // 8 of the delay (the scan is in the docstring)
NOISY = {(1200, 3000.0): 1.0, (9600, 12000.0): 0.2}
# the seeds whose capture decodes without bit timing all the same, at that sigma (on the restatement)
UNACQUIRED_OK = {1200: {3, 6, 8, 9}, 9600: {2, 4, 5, 6, 8, 10}}


@pytest.fixture(scope="module")
def product(built_lib):
    """The restatement is only worth testing beside the product it restates."""
    import _amr
    import modem
    for name in ("minshift_modulate", "minshift_demodulate", "minshift_demodulate_batch", "minshift_demodulate_soft",
                 "minshift_demodulate_soft_batch", "minshift_acquire", "minshift_acquire_batch"):
        assert callable(getattr(modem, name)), name
    for name in ("msk_geometry", "design_msk", "MskPlan", "get_msk_plan", "msk_tx_samples", "msk_modulate",
                 "msk_slice", "msk_soft"):
        assert callable(getattr(_amr, name)), name
    assert _amr.MskPlan._slots == _amr.TD_SLOTS == ["despread", "slice", "sync_pack", "launch", "acquire"]
    return _amr.lib()


def payload(rng, n):
    return b"FBPC" + rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def recovered(data, sync, msg):
    """The sync word was found and the payload follows it (what lies behind it is the closing bit and the tail)."""
    return sync >= 0 and data[:len(msg)] == msg


def round_trips(baud, carrier, fs, rng, n_payload, delays=3):
    """The aligned clean capture comes back exactly, sync at bit 80; from random delays below 3 L, digital
    silence before and 2 L after, a clean capture gives o == t % L exactly and its payload."""
    L, h, cyc4 = mc.geometry(baud, carrier, fs)
    msg = payload(rng, n_payload)
    w = mc.modulate(msg, baud, carrier, fs)
    assert w.dtype == np.float32 and w.size == (82 + 8 * len(msg)) * L
    data, sync, o = mc.demod(w, baud, carrier, fs, acquire_=False)
    assert (data, sync, o) == (msg, mc.SYNC_AT, 0), (L, cyc4)
    sdata, soft, ssync, _ = mc.demod_soft(w, baud, carrier, fs, acquire_=False)
    assert (sdata, ssync) == (data, sync) and np.packbits(soft > 0).tobytes() == data
    for _ in range(delays):
        t = int(rng.integers(0, 3 * L))
        x = mc.delayed(msg, t, baud, carrier, samp_rate=fs)
        assert x.size == t + w.size + 2 * L
        o, q = mc.acquire(x, baud, carrier, fs)
        assert o == t % L, (L, cyc4, t, o)
        data, sync, o2 = mc.demod(x, baud, carrier, fs)
        assert o2 == o and recovered(data, sync, msg) and sync == mc.SYNC_AT + t // L, (L, cyc4, t)


@pytest.mark.parametrize("baud,carrier", oc.CONFIGS)
def test_aligned_and_delayed_round_trips(product, baud, carrier):
    rng = np.random.default_rng(int(baud))
    L, h, cyc4 = mc.geometry(baud, carrier)
    assert L == 96000 // baud and h == L // 2 and cyc4 == round(4 * carrier * L / 96000)
    round_trips(baud, carrier, 96000, rng, int(rng.integers(20, 61)))


def test_the_constant_envelope_and_the_continuous_phase(product):
    """What makes it MSK: every sample is a table sine of one running integer phase, whose step from sample to
    sample is cyc4 + 1 or cyc4 - 1 units of 1 / (4 L) cycle, also across a bit boundary; the tones are half
    the bit rate apart."""
    import _amr
    baud, carrier = 9600, 12000.0
    L, h, cyc4, Sn, *_ = _amr.design_msk(baud, carrier)
    msg = payload(np.random.default_rng(1), 9)
    w = mc.modulate(msg, baud, carrier)
    bits = mc.tx_bits(msg).astype(np.int64)
    assert bits.size == 82 + 8 * len(msg) and bits[0] == 0 and bits[-1] == 0 and bits[1:81].tolist() == mc.PREAMBLE
    inc = np.repeat(cyc4 + 2 * bits - 1, L)
    phase = np.concatenate([[0], np.cumsum(inc)[:-1]]) % (4 * L)
    assert np.array_equal(w, Sn[phase].astype(np.float32))
    f1, f0 = (cyc4 + 1) * 96000 / (4 * L), (cyc4 - 1) * 96000 / (4 * L)
    assert f1 - f0 == baud / 2 and (f1 + f0) / 2 == carrier


def test_the_smallest_bit_and_a_carrier_on_a_quarter_of_the_sample_rate(product):
    rng = np.random.default_rng(4)
    round_trips(*mc.pair_of(4, 2), rng, 12)                  # L = 4, the lowest carrier
    round_trips(*mc.pair_of(4, 6), rng, 12)                  # L = 4, the highest: cyc4 + 1 = 2 L - 1
    for L in (4, 7, 10, 33):                                 # cyc4 = L: the carrier on fs / 4
        b, c, fs = mc.pair_of(L, L)
        assert c == fs / 4
        round_trips(b, c, fs, rng, 12)


def test_every_valid_geometry_up_to_twelve_samples_per_bit(product):
    """Every (L, cyc4) with 4 <= L <= 12, 2 <= cyc4 and cyc4 + 1 < 2 L: aligned and from three delays, clean."""
    pairs = mc.valid_pairs(12)
    assert len(pairs) == sum(2 * L - 3 for L in range(4, 13)) and (4, 2) in pairs and (12, 22) in pairs
    assert {c % 4 for L, c in pairs} == {0, 1, 2, 3}
    rng = np.random.default_rng(12)
    for L, cyc4 in pairs:
        round_trips(*mc.pair_of(L, cyc4), rng, 8)


@pytest.mark.parametrize("baud,carrier", list(NOISY))
def test_noise(product, baud, carrier):
    """Every one of the 12 seeded captures, delayed at random, gives its payload back with o within L // 8 of the
    delay, circularly.  Scan on the restatement (payloads recovered of 12; every o was within L // 8 at every
    sigma): at 1200 Bd (L = 80) 12 from 0.2 to 1.0, 10 at 1.1, 9 at 1.2 -> sigma 1.0; at 9600 Bd (L = 10) 12
    at 0.2, 10 at 0.3, 4 at 0.4, 0 from 0.5 on -> sigma 0.2: a bit of 10 samples integrates an eighth of
    the energy.  What fails first is the differential decision, never the bit timing.  Unacquired, the same
    captures fail except where UNACQUIRED_OK says."""
    sigma = NOISY[baud, carrier]
    L = mc.geometry(baud, carrier)[0]
    for seed in range(TRIALS):
        rng = np.random.default_rng(1000 * seed + int(baud))
        msg = payload(rng, int(rng.integers(20, 61)))
        t = int(rng.integers(0, 3 * L))
        x = mc.delayed(msg, t, baud, carrier, sigma=sigma, rng=rng)
        data, sync, o = mc.demod(x, baud, carrier)
        assert recovered(data, sync, msg), (seed, t, o)
        assert min((o - t) % L, (t - o) % L) <= L // 8, (seed, t, o)
        plain = mc.demod(x, baud, carrier, acquire_=False)
        assert recovered(*plain[:2], msg) == (seed in UNACQUIRED_OK[baud]), seed


def test_invalid_geometries(product):
    import _amr
    import modem
    g = _amr.msk_geometry
    assert g(9600, 12000.0) == (10, 5, 5) and g(1200, 3000.0) == (80, 40, 10)
    assert g(24000, 12000.0) == (4, 2, 2) and g(9600, 43200.0) == (10, 5, 18)       # 18 + 1 < 2 L: the highest cyc4
    bad = [
        dict(baud=32000),                                    # L = 3
        dict(baud=48000), dict(baud=200000),                 # L = 2, 0
        dict(carrier=3000.0),                                # cyc4 = floor(4 * 3000 * 10 / 96000 + 0.5) = 1
        dict(carrier=100.0),                                 # cyc4 = 0
        dict(carrier=45600.0), dict(carrier=48000.0),        # cyc4 = 19, 20: cyc4 + 1 >= 2 L
        dict(baud=0.001),                                    # L > 2^24
    ]
    assert g(9600, 44300.0)[2] == 18                         # 18.46 rounds to 18: valid ...
    with pytest.raises(ValueError):
        g(9600, 44500.0)                                     # ... and 18.54 to 19: not
    for kw in bad:
        args = dict(baud=9600, carrier=12000.0)
        args.update(kw)
        with pytest.raises(ValueError):
            g(args["baud"], args["carrier"])
        with pytest.raises(ValueError):                      # before any device work: no GPU is needed to refuse
            modem.minshift_demodulate(np.zeros(4000, np.float32), args["baud"], args["carrier"])
        with pytest.raises(ValueError):
            modem.minshift_modulate(b"x", args["baud"], args["carrier"])
        with pytest.raises(ValueError):
            modem.minshift_acquire_batch(np.zeros((0, 10), np.float32), args["baud"], args["carrier"])
        with pytest.raises(ValueError):
            modem.modulate_batch("minshift", [b"x"], args["baud"], args["carrier"])
    # the C side refuses the same before any device work
    L = product
    h = ctypes.c_void_p()
    Lb, hb, cyc4, Sn, U, E0, E1, R = _amr.design_msk(9600, 12000.0)
    p = _amr.ptr
    inv = _amr.AMR_E_INVALID
    create = L.amr_msk_plan_create
    tabs = (p(U), p(E0), p(E1), p(R))
    assert create(ctypes.byref(h), 0, 1000, 3, 2, *tabs, 1) == inv
    assert create(ctypes.byref(h), 0, 1000, 10, 1, *tabs, 1) == inv
    assert create(ctypes.byref(h), 0, 1000, 10, 19, *tabs, 1) == inv
    assert b"upper tone" in L.amr_last_error()
    assert create(ctypes.byref(h), 0, 1000, (1 << 24) + 1, 5, *tabs, 1) == inv
    assert create(ctypes.byref(h), 0, -1, 10, 5, *tabs, 1) == inv
    assert create(ctypes.byref(h), 0, 1000, 10, 5, *tabs, 0) == inv
    for k in range(4):
        t = list(tabs)
        t[k] = None
        assert create(ctypes.byref(h), 0, 1000, 10, 5, *t, 1) == inv
    assert create(None, 0, 1000, 10, 5, *tabs, 1) == inv


def test_the_bit_rule_and_the_soft_signs_are_total(product):
    nan, inf = np.nan, np.inf
    vals = [0.0, -0.0, 1.0, -1.0, 2.0 ** 500, -2.0 ** 500, 2.0 ** -500, -2.0 ** -500, 5e-324, -5e-324, inf, -inf, nan]
    D = np.array([complex(a, b) for a in vals for b in vals])
    bits = mc.bits_of_products(D)
    assert bits.dtype == np.uint8 and set(bits.tolist()) == {0, 1}
    assert np.array_equal(bits == 1, np.array([b > 0 for _ in vals for b in vals]))
    assert bits[np.isnan(D.imag)].sum() == 0 and bits[D.imag == 0].sum() == 0
    s = mc.soft_of_products(D)
    assert s.dtype == np.int8 and np.array_equal(s > 0, bits == 1)
    assert np.all((np.abs(s.astype(int)) >= 1) & (np.abs(s.astype(int)) <= 127))
    # through the product model and the quarter-turns: the soft sign is the hard bit at every scale and rotation
    rng = np.random.default_rng(4)
    for cyc4, scale in zip((4, 5, 6, 7), (1.0, 2.0 ** 500, 2.0 ** -500, 2.0 ** -530)):
        W = (rng.standard_normal(200) + 1j * rng.standard_normal(200)) * scale
        W[7] = 0.0
        W[50] = complex(nan, 1.0)
        W[90] = complex(inf, -inf)
        b, s = mc.slice_bits(W, cyc4), mc.soft(W, cyc4)
        assert b.shape == s.shape == (199,) and np.array_equal(s > 0, b == 1)
        assert b[6] == b[7] == 0 and s[6] == s[7] == -1      # a zero window: the product is zero, the bit 0, magnitude 1
        assert b[49] == b[50] == 0                           # a NaN component: 0
    # the four rotations of one product: (-i)^r turns 1 + 2i into 1 + 2i, 2 - i, -1 - 2i, -2 + i
    W = np.array([1.0, 1.0 + 2.0j])
    assert [complex(mc.products(W, r)[0]) for r in range(4)] == [1 + 2j, 2 - 1j, -1 - 2j, -2 + 1j]
    assert mc.slice_bits(np.zeros(1, np.complex128), 5).size == 0 and mc.soft(np.zeros(0, np.complex128), 5).size == 0


def test_the_timing_rule_is_total(product):
    import _amr
    baud, carrier = 9600, 12000.0
    L = 10
    R = _amr.design_msk(baud, carrier)[7]
    nan, inf = np.nan, np.inf
    # n = 0, all zeros: q = 0, every P is 0, nothing is above P[0]
    for x in (np.zeros(0, np.float32), np.zeros(1000, np.float32), np.zeros(5000, np.int16)):
        o, q = mc.acquire(x, baud, carrier)
        assert o == 0 and q == 0
        assert mc.segment_sums(x, baud, carrier).shape == (-(-x.size // 4096), 4)
    # a NaN or an infinity anywhere in x is in both line sums: q is NaN, P[0] is NaN, 0 is kept
    rng = np.random.default_rng(9)
    msg = payload(rng, 60)
    for k, v in ((0, nan), (4321, nan), (77, inf), (5000, -inf)):    # the first segment and the second
        x = mc.delayed(msg, 7, baud, carrier)
        assert x.size > 5000
        assert mc.acquire(x, baud, carrier)[0] == 7
        x[k] = v
        with np.errstate(all="ignore"):
            o, q = mc.acquire(x, baud, carrier)
        assert o == 0 and np.isnan(q.real), (k, v)
    # the score on crafted sums: an exact tie takes the first index; q = 0 and a NaN q give 0
    q, P = mc.score(complex(1.0, 0.0), complex(0.0, 0.0), R)
    assert q == 0 and not P.any() and mc.first_max(P) == 0
    q, P = mc.score(complex(1.0, 0.0), complex(-1.0, 0.0), R)          # q = -1: P[d] = -cos(2 pi d / L), largest at L / 2
    assert q == -1 and mc.first_max(P) == 5
    q, P = mc.score(complex(1.0, 0.0), complex(nan, 0.0), R)
    assert np.isnan(P).all() and mc.first_max(P) == 0
    assert mc.offset_of(complex(1.0, 0.0), complex(-1.0, 0.0), baud, carrier)[0] == 5
    # short captures: Sw < 2 gives b"", sync -1
    for n in (0, 1, 14, 15, 24):                             # (n + 5) // 10 - 1 = 0, 0, 0, 1, 1
        assert mc.n_windows(n, L) < 2
        assert mc.demod(np.ones(n, np.float32), baud, carrier)[:2] == (b"", -1)
        assert mc.demod_soft(np.ones(n, np.float32), baud, carrier, acquire_=False)[0] == b""
    assert mc.n_windows(25, L) == 2 and mc.n_windows(0, L) == 0


def test_the_summation_order_is_part_of_the_definition(product):
    """Two segments and a short third: the lines are the segments' tree sums added in order, not one running sum."""
    import _amr
    baud, carrier = 9600, 12000.0
    L, h, cyc4, Sn, U, E0, E1, R = _amr.design_msk(baud, carrier)
    rng = np.random.default_rng(2)
    x = rng.standard_normal(2 * 4096 + 100)
    g = mc.segment_sums(x, baud, carrier)
    assert g.shape == (3, 4)
    sq = x * x
    v = sq * E1[np.arange(x.size) % (2 * L), 0]
    want = []
    for s in range(3):
        seg = v[4096 * s:4096 * (s + 1)]
        p = np.zeros(64)
        for a in range(0, seg.size, 64):
            row = seg[a:a + 64]
            p[:row.size] = p[:row.size] + row
        for w in (32, 16, 8, 4, 2, 1):
            p[:w] = p[:w] + p[w:2 * w]
        want.append(p[0])
    assert g[:, 2].tolist() == want
    c0, c1 = mc.lines(x, baud, carrier)
    assert c1.real == (0.0 + want[0] + want[1]) + want[2] and c1.real != np.sum(v)


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
    q = np.zeros((1, 2))
    W = np.zeros((1, 5, 2))
    words = np.zeros((1, 1), np.uint32)
    assert L.amr_msk_demod_host(None, p(x), 0, 1, 400, p(out), 64, p(ln), p(sy), p(soft), 512, p(of), 1) == inv
    assert b"amr_msk_demod_host" in L.amr_last_error()
    assert L.amr_msk_demod_device(None, p(x), 0, 1, 400, p(out), 64, p(ln), p(sy), None, 0, None, 0) == inv
    assert L.amr_msk_demod_host(None, p(x), 0, -1, 400, p(out), 64, p(ln), p(sy), None, 0, None, 1) == inv
    assert b"negative" in L.amr_last_error()
    assert L.amr_msk_acquire_host(None, p(x), 0, 1, 400, p(of), p(q)) == inv
    assert b"amr_msk_acquire_host" in L.amr_last_error()
    assert L.amr_msk_acquire_device(None, p(x), 0, 1, 400, p(of), None) == inv
    assert L.amr_msk_symbols_at_host(None, p(x), 0, 1, 400, p(of), p(W)) == inv
    assert L.amr_msk_slice_host(p(W), 1, 5, 5, None) == inv and L.amr_msk_slice_host(None, 1, 5, 5, p(words)) == inv
    assert L.amr_msk_soft_host(p(W), 1, 5, 5, None) == inv and L.amr_msk_soft_host(p(W), -1, 5, 5, p(soft)) == inv
    assert L.amr_msk_slice_host(p(W), 1, 5, -1, p(words)) == inv
    assert L.amr_msk_slice_host(None, 0, 0, 5, None) == _amr.AMR_OK and L.amr_msk_soft_host(p(W), 1, 1, 5, p(soft)) == _amr.AMR_OK
    assert L.amr_msk_plan_out_capacity(None) == -1 and L.amr_msk_plan_scratch_bytes(None) == -1
    assert L.amr_msk_plan_synchronize(None) == inv and L.amr_msk_plan_enable_timing(None, 1) == inv
    assert L.amr_msk_plan_timings(None, None, 5) == inv and L.amr_msk_plan_destroy(None) == _amr.AMR_OK
    # the score stage's checks
    Lb, hb, cyc4, Sn, U, E0, E1, R = _amr.design_msk(9600, 12000.0)
    c = np.zeros((1, 4))
    assert L.amr_msk_offset_host(10, None, p(c), 1, p(of), p(q)) == inv
    assert L.amr_msk_offset_host(10, p(R), None, 1, p(of), p(q)) == inv
    assert L.amr_msk_offset_host(10, p(R), p(c), 1, None, p(q)) == inv
    assert L.amr_msk_offset_host(3, p(R), p(c), 1, p(of), p(q)) == inv
    assert L.amr_msk_offset_host(10, p(R), p(c), -1, p(of), p(q)) == inv
    assert L.amr_msk_offset_host(10, p(R), None, 0, None, None) == _amr.AMR_OK
    # the modulator's checks
    nb = np.array([3], np.int64)
    data = np.zeros((1, 3), np.uint8)
    o32 = np.zeros((1, 100), np.float32)
    mod = L.amr_msk_modulate_host
    assert mod(10, 5, p(Sn), p(data), 3, p(nb), 1, p(o32), 99, 100, None, 0) == inv     # out_stride < n_out
    assert mod(10, 5, None, p(data), 3, p(nb), 1, p(o32), 100, 100, None, 0) == inv
    assert mod(10, 1, p(Sn), p(data), 3, p(nb), 1, p(o32), 100, 100, None, 0) == inv
    assert mod(3, 2, p(Sn), p(data), 3, p(nb), 1, p(o32), 100, 100, None, 0) == inv
    assert mod(10, 5, p(Sn), p(data), 2, p(nb), 1, p(o32), 100, 100, None, 0) == inv    # n_bytes > stride
    assert mod(10, 5, p(Sn), None, 0, None, 0, None, 0, 0, None, 0) == _amr.AMR_OK       # empty batch
    # the byte estimates are host arithmetic
    est, acq = L.amr_msk_plan_bytes_estimate, L.amr_msk_acquire_bytes_estimate
    assert acq(96000, 10, 1) == 24 * 32 + 16 + 8                           # 24 segments of four doubles, q, the offset
    assert acq(96000, 10, 4096) == 4096 * acq(96000, 10, 1)
    assert acq(0, 10, 2) == 32 + 2 * (16 + 8)                               # no segment
    assert acq(96000, 3, 1) < 0 and acq(96000, 10, 0) < 0 and acq(-1, 10, 1) < 0
    e1, e2 = est(96000, 10, 1), est(96000, 10, 64)
    assert 0 < e1 < e2 < 64 * e1 + 1 and est(96000, 3, 1) < 0 and est(96000, 10, 0) < 0
    assert _amr.msk_tx_samples(7, 9600, 12000.0) == (82 + 56) * 10
    if _amr.device_count() < 1:
        z = np.zeros(4000, np.float32)
        for call in (lambda: modem.minshift_acquire(z, 9600, 12000.0), lambda: modem.minshift_demodulate(z, 9600, 12000.0),
                     lambda: modem.minshift_demodulate_soft(z, 9600, 12000.0, acquire=False),
                     lambda: modem.minshift_modulate(b"FBPC", 9600, 12000.0),
                     lambda: modem.modulate_batch("minshift", [b"a"], 9600, 12000.0),
                     lambda: _amr.msk_slice(np.ones((1, 3), np.complex128), 5),
                     lambda: _amr.msk_soft(np.ones((1, 3), np.complex128), 5)):
            with pytest.raises(_amr.AmrError):
                call()
    with pytest.raises(ValueError):
        modem.minshift_acquire(np.zeros((2, 4000), np.float32), 9600, 12000.0)
    with pytest.raises(ValueError):
        modem.minshift_demodulate(np.zeros((2, 4000), np.float32), 9600, 12000.0)
    assert modem.minshift_acquire_batch(np.zeros((0, 100), np.float32), 9600, 12000.0).shape == (0,)
    assert modem.minshift_demodulate_batch(np.zeros((0, 100), np.float32), 9600, 12000.0) == []
    assert modem.minshift_demodulate_soft_batch(np.zeros((0, 100), np.float32), 9600, 12000.0) == ([], [])


def test_the_alias_is_untouched(product):
    """msk_modulate stays the reference's FSK call with tone spacing baud: same function body, nothing minshift."""
    import inspect
    import modem
    src = inspect.getsource(modem.msk_modulate)
    assert "fsk_modulate" in src and "minshift" not in src
